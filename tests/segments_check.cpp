// segments_check.cpp -- the host side of gen.simuSegments (csrc/link_segments.h) as a stand-alone program: built by
// tests/test_segments_host.py with g++, plain and under AddressSanitizer + UndefinedBehaviorSanitizer, from the header alone.  The
// walk over the words of a chromosome (seg_walk_word through seg_reduce_host) is checked against a loop over single bits on random
// chromosomes of every density and of the lengths at the word edges, the bin of a length against a linear search, and seg_sizes,
// seg_cells, seg_lds_bytes and the check of a request against their formulas on random requests.  Prints one summary line; exit
// status 1 on any violation.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../genlib.jl_amd/csrc/link_segments.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
int64_t below(int64_t n) { return static_cast<int64_t>(rnd() % static_cast<uint64_t>(n)); }

long violations = 0;
void expect(bool ok, const char *what, long at)
{
    if (ok) return;
    ++violations;
    std::fprintf(stderr, "VIOLATION in case %ld: %s\n", at, what);
}

// a word whose bits are set with probability num / 64
uint64_t word_of_density(int num)
{
    uint64_t w = 0;
    for (int k = 0; k < 64; ++k)
        if (below(64) < num) w |= 1ull << k;
    return w;
}

// the definition, one bit at a time
void literal(int L, const std::vector<uint64_t> &words, const std::vector<int32_t> &edges, int min_loci, std::vector<int64_t> &hist, int64_t pair[3],
             long &runs, long &crossing)
{
    int open = 0, longest = 0;
    for (int k = 0; k <= L; ++k) {
        const bool bit = k < L && ((words[k / 64] >> (k % 64)) & 1);
        if (bit) {
            ++open;
            continue;
        }
        if (!open) continue;
        const int start = k - open;
        int col = 0;
        for (size_t e = 0; e < edges.size(); ++e) col += edges[e] <= open;
        hist[3 * col] += 1;
        hist[3 * col + 1] += open;
        hist[3 * col + 2] += start == 0 || k == L;
        if (open >= min_loci) {
            pair[0] += 1;
            pair[1] += open;
        }
        if (open > longest) longest = open;
        ++runs;
        crossing += start / 64 != (k - 1) / 64;
        open = 0;
    }
    pair[2] += longest;
}

}  // namespace

int main()
{
    const int lengths[] = {1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1000, 4095, 4096};
    const int densities[] = {0, 1, 8, 32, 56, 63, 64};
    long cases = 0, runs = 0, crossing = 0, bits = 0;
    for (long c = 0; c < 100000; ++c, ++cases) {
        const int L = c % 4 ? lengths[below(9)] : (c % 64 ? lengths[below(14)] : 1 + static_cast<int>(below(4096)));
        const int W = (L + 63) / 64;
        std::vector<uint64_t> words(W);
        const int kind = static_cast<int>(below(10));
        const int density = densities[below(7)];
        for (int w = 0; w < W; ++w) {
            if (kind == 0) words[w] = below(2) ? ~0ull : 0ull;                       // whole words: runs that end and start at word borders
            else if (kind == 1) words[w] = word_of_density(densities[below(7)]);    // a density per word
            else if (kind == 2) words[w] = below(3) ? ~0ull : word_of_density(60);  // long runs over many words
            else words[w] = word_of_density(density);
        }
        if (below(2)) words[W - 1] |= rnd() << 1;                                    // bits at and above L are ignored
        int n_edges = 2 + static_cast<int>(below(below(8) ? 6 : 256));
        std::vector<int32_t> edges;
        {
            // n_edges strictly increasing values in 1 .. 4097 (fewer when the draw runs out of room)
            int32_t v = 1 + static_cast<int32_t>(below(3));
            for (int e = 0; e < n_edges && v <= genphi::kSegMaxEdge; ++e) {
                edges.push_back(v);
                v += 1 + static_cast<int32_t>(below(below(4) ? 4 : 1 + 2 * L / n_edges));
            }
            if (edges.size() < 2) edges = {1, 2};
            n_edges = static_cast<int>(edges.size());
        }
        const int min_loci = 1 + static_cast<int>(below(below(2) ? 4 : L + 1));
        expect(genphi::seg_check_request(n_edges, edges.data(), min_loci, 0, nullptr, 0).empty(), "a valid request is refused", c);
        std::vector<int64_t> want(3 * (n_edges + 1), 0), got(3 * (n_edges + 1), 0);
        int64_t want_pair[3] = {0, 0, 0}, got_pair[3] = {0, 0, 0};
        literal(L, words, edges, min_loci, want, want_pair, runs, crossing);
        genphi::seg_reduce_host(L, words.data(), n_edges, edges.data(), min_loci, got.data(), got_pair);
        expect(want == got, "the table of the walk differs from the bit loop's", c);
        expect(want_pair[0] == got_pair[0] && want_pair[1] == got_pair[1] && want_pair[2] == got_pair[2], "the pair sums of the walk differ", c);
        // both outputs are added to, and either may be missing
        genphi::seg_reduce_host(L, words.data(), n_edges, edges.data(), min_loci, got.data(), nullptr);
        genphi::seg_reduce_host(L, words.data(), n_edges, edges.data(), min_loci, nullptr, got_pair);
        bool twice = got_pair[0] == 2 * want_pair[0] && got_pair[1] == 2 * want_pair[1] && got_pair[2] == 2 * want_pair[2];
        for (size_t k = 0; k < want.size(); ++k) twice = twice && got[k] == 2 * want[k];
        expect(twice, "a second reduction does not add to the first", c);
        for (int len = 1; len <= L && len <= 300; len += 1 + static_cast<int>(below(7))) {
            int col = 0;
            for (int e = 0; e < n_edges; ++e) col += edges[e] <= len;
            expect(genphi::seg_bin(edges.data(), n_edges, len) == col, "seg_bin differs from the linear count", c);
        }
        bits += L;
    }
    // requests: sizes, cells and the cell limit
    long requests = 0, refused = 0;
    for (long c = 0; c < 600; ++c, ++requests) {
        const int32_t n_groups = static_cast<int32_t>(below(36)) - 1 + (c % 7 == 0);
        const int32_t n_edges = static_cast<int32_t>(c % 3 ? 2 + below(40) : 2 + below(258));
        const int64_t n_pro = 1 + below(c % 5 ? 50 : 40000);
        std::vector<int32_t> edges(n_edges > 0 ? n_edges : 0);
        for (int32_t e = 0; e < n_edges; ++e) edges[e] = 1 + e * (4096 / n_edges);
        std::vector<int32_t> group(n_pro);
        for (auto &g : group) g = n_groups > 0 ? static_cast<int32_t>(below(n_groups + 1)) - 1 : 0;
        const int64_t G = n_groups > 1 ? n_groups : 1;
        const int64_t cells = G * (G + 1) / 2 * (n_edges + 1);
        const bool fits = n_groups >= 0 && n_groups <= 32 && n_edges <= 257 && cells <= 2048;
        const std::string err = genphi::seg_check_request(n_edges, edges.data(), 1, n_groups, group.data(), n_pro);
        expect(err.empty() == fits, "the check of a request and the limits disagree", c);
        refused += !err.empty();
        if (!fits) continue;
        expect(genphi::seg_cells(n_edges, n_groups) == cells, "seg_cells", c);
        const genphi::SegSizes z = genphi::seg_sizes(n_pro, n_edges, n_groups);
        expect(z.table == static_cast<size_t>(24 * cells) && z.pairs == static_cast<size_t>(24 * n_pro * n_pro) && z.edges == static_cast<size_t>(4 * n_edges) &&
                   z.labels == static_cast<size_t>(4 * n_pro) && z.fixed() == z.table + z.pairs + z.edges + z.labels,
               "seg_sizes", c);
        const int32_t planes = 1 + static_cast<int32_t>(below(16));
        expect(genphi::seg_lds_bytes(planes, n_edges, n_groups) == static_cast<size_t>(2048 * planes + 24 * cells + 4 * n_edges), "seg_lds_bytes", c);
        expect(genphi::seg_lds_bytes(planes, n_edges, n_groups) <= 160 * 1024, "the LDS of a workgroup exceeds 160 KiB", c);
        // every pair of groups has a cell of its own, a <= b row after row
        int32_t next = 0;
        bool dense = true;
        for (int32_t a = 0; a < G; ++a)
            for (int32_t b = a; b < G; ++b) dense = dense && genphi::seg_group_pair(a, b, static_cast<int32_t>(G)) == next++ && genphi::seg_group_pair(b, a, static_cast<int32_t>(G)) == next - 1;
        expect(dense && next == G * (G + 1) / 2, "seg_group_pair is not the upper triangle row after row", c);
    }
    expect(genphi::seg_sizes(100, 0, 0).fixed() == 0, "no request holds no bytes", 0);
    // the limits themselves.  G (G + 1) / 2 x (n_edges + 1) never is 2048 or 2049 with 2 .. 257 edges (2048 is a power of two and 1 the only
    // triangular one, 2049 = 3 x 683): the largest request that passes has 2046 cells (11 groups, 30 edges), the smallest refused 2050 (4, 204)
    {
        std::vector<int32_t> edges(257);
        for (int e = 0; e < 257; ++e) edges[e] = 1 + e;
        std::vector<int32_t> group(4, 0);
        bool reach = false;
        for (int32_t G = 1; G <= 32; ++G)
            for (int32_t n = 2; n <= 257; ++n) {
                const int64_t cells = genphi::seg_cells(n, G);
                reach = reach || cells == 2047 || cells == 2048 || cells == 2049;
                expect(genphi::seg_check_request(n, edges.data(), 1, G, group.data(), 4).empty() == (cells <= 2048), "the cell limit is not 2048", G * 1000 + n);
            }
        expect(!reach, "2047, 2048 or 2049 cells can be reached after all", 0);
        expect(genphi::seg_cells(30, 11) == 2046 && genphi::seg_check_request(30, edges.data(), 1, 11, group.data(), 4).empty(), "2046 cells are refused", 0);
        expect(genphi::seg_cells(204, 4) == 2050 && !genphi::seg_check_request(204, edges.data(), 1, 4, group.data(), 4).empty(), "2050 cells pass", 0);
        expect(!genphi::seg_check_request(2, edges.data(), 1, 33, group.data(), 4).empty(), "33 groups pass", 0);
        expect(!genphi::seg_check_request(258, edges.data(), 1, 0, nullptr, 4).empty() && !genphi::seg_check_request(1, edges.data(), 1, 0, nullptr, 4).empty(), "258 edges or 1 edge pass", 0);
        group[2] = 3;
        expect(!genphi::seg_check_request(4, edges.data(), 1, 3, group.data(), 4).empty(), "a label of 3 with 3 groups passes", 0);
        group[2] = -2;
        expect(!genphi::seg_check_request(4, edges.data(), 1, 3, group.data(), 4).empty(), "a label of -2 passes", 0);
        group[2] = -1;
        expect(genphi::seg_check_request(4, edges.data(), 1, 3, group.data(), 4).empty(), "a label of -1 is refused", 0);
        edges[3] = edges[2];
        expect(!genphi::seg_check_request(5, edges.data(), 1, 0, nullptr, 4).empty(), "equal edges pass", 0);
        edges[3] = 4;
        edges[0] = 0;
        expect(!genphi::seg_check_request(5, edges.data(), 1, 0, nullptr, 4).empty(), "an edge of 0 passes", 0);
        edges[0] = 1;
        edges[4] = 4098;
        expect(!genphi::seg_check_request(5, edges.data(), 1, 0, nullptr, 4).empty(), "an edge of 4098 passes", 0);
        edges[4] = 4097;
        expect(genphi::seg_check_request(5, edges.data(), 4097, 0, nullptr, 4).empty(), "an edge of 4097 and min_loci = 4097 are refused", 0);
        expect(!genphi::seg_check_request(5, edges.data(), 4098, 0, nullptr, 4).empty() && !genphi::seg_check_request(5, edges.data(), 0, 0, nullptr, 4).empty(), "min_loci of 0 or 4098 passes", 0);
    }
    std::printf("segments check: %ld cases, %ld loci, %ld runs, %ld crossing a word, %ld requests, %ld refused; %ld violations\n", cases, bits, runs, crossing,
                requests, refused, violations);
    return violations ? 1 : 0;
}
