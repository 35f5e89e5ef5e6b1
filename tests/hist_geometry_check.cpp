// hist_geometry_check.cpp -- the host arithmetic of genphi_result_hist / genphi_result_select (csrc/hist_geometry.h) held to its
// invariants without a GPU (tests/test_phi_hist_host.py builds this with g++, plainly and under AddressSanitizer +
// UndefinedBehaviorSanitizer):
//   walks   for N in {1, 2, 3, 64, 65, 1025, 100000, 1500000}, row shards, label patterns, numbers of chunks asked for and pair
//           limits: `order` is exactly the rows that can hold a counted pair, sorted by (label, row); the chunks partition it, none is
//           empty, each holds fewer pairs than the limit (2^31 by default); the pairs add up to the closed form; no more chunks than
//           asked for unless the limit forces them; the scratch block of the call is aligned, ordered and large enough;
//   edges   for doubles around Float32 values (between two of them, on one, one Float64 step off, +-inf, beyond FLT_MAX, below the
//           smallest subnormal): comparing a Float32 x with hist_float_at_or_above(e) / hist_float_above(e) decides as (double)x >= e
//           / (double)x > e for the Float32 values around e; the count over hist_thresholds is the bin of the Float64 definition;
//   limits  the LDS request of every allowed (edges, groups) stays within 160 KiB.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../genlib.jl_amd/csrc/hist_geometry.h"

namespace {

long long g_checks = 0, g_violations = 0, g_walks = 0, g_edges = 0;

void expect(bool ok, const char *what, long long a = 0, long long b = 0, long long c = 0)
{
    ++g_checks;
    if (!ok) {
        ++g_violations;
        if (g_violations <= 20) std::fprintf(stderr, "VIOLATION: %s (%lld, %lld, %lld)\n", what, a, b, c);
    }
}

// pattern 0: no labels; 1: two runs; 2: k % 3, every fifth unlabelled; 3: one group; 4: all unlabelled; 5: 256 groups interleaved
std::vector<int32_t> labels_of(int pattern, int64_t n, int *n_groups)
{
    std::vector<int32_t> lab(static_cast<size_t>(n));
    *n_groups = pattern == 1 ? 2 : pattern == 2 ? 3 : pattern == 5 ? 256 : 1;
    for (int64_t k = 0; k < n; ++k) {
        int32_t g = 0;
        if (pattern == 1) g = k < n / 2 ? 1 : 0;                       // (the later run has the smaller label)
        if (pattern == 2) g = k % 5 == 0 ? -1 : static_cast<int32_t>(k % 3);
        if (pattern == 4) g = -1;
        if (pattern == 5) g = static_cast<int32_t>((k * 7) % 256);
        lab[static_cast<size_t>(k)] = g;
    }
    return lab;
}

void check_walk(int64_t n, int64_t r0, int64_t r1, int pattern, int64_t want, int64_t limit)
{
    ++g_walks;
    int G = 0;
    std::vector<int32_t> lab;
    if (pattern) lab = labels_of(pattern, n, &G);
    const int32_t *group = pattern ? lab.data() : nullptr;
    const genphi::HistChunks h = genphi::hist_chunks(n, r0, r1, group, G, want, limit);
    // the rows that can hold a counted pair
    int64_t eligible = 0, pairs = 0;
    for (int64_t i = r0; i < r1 && i < n - 1; ++i)
        if (!group || group[i] >= 0) { ++eligible; pairs += genphi::hist_row_pairs(n, i); }
    expect(static_cast<int64_t>(h.order.size()) == eligible, "order holds the eligible rows", n, r0, r1);
    expect(h.pairs == pairs, "pairs of the walk", n, h.pairs, pairs);
    if (!group) expect(pairs == genphi::hist_pairs_of_rows(n, r0, r1),
                       "closed form of the pairs", n, r0, r1);
    for (size_t p = 0; p < h.order.size(); ++p) {
        const int64_t i = h.order[p];
        expect(i >= r0 && i < r1 && i < n - 1 && (!group || group[i] >= 0), "a row of the order is eligible", n, i);
        if (p) {
            const int64_t q = h.order[p - 1];
            const int ga = group ? group[q] : 0, gb = group ? group[i] : 0;
            expect(ga < gb || (ga == gb && q < i), "sorted by (label, row), no row twice", n, q, i);
        }
    }
    if (h.order.empty()) {
        expect(h.n_chunks() == 0, "no row, no chunk", n);
    } else {
        expect(h.n_chunks() >= 1 && h.begin.front() == 0 && h.begin.back() == static_cast<int32_t>(h.order.size()), "the chunks cover the order", n);
        int64_t sum = 0;
        bool forced = false;
        for (int c = 0; c < h.n_chunks(); ++c) {
            expect(h.begin[static_cast<size_t>(c)] < h.begin[static_cast<size_t>(c) + 1], "no empty chunk", n, c);
            int64_t w = 0;
            for (int32_t p = h.begin[static_cast<size_t>(c)]; p < h.begin[static_cast<size_t>(c) + 1]; ++p) w += genphi::hist_row_pairs(n, h.order[static_cast<size_t>(p)]);
            expect(w < limit, "a chunk holds fewer pairs than the limit", n, c, w);
            if (c + 1 < h.n_chunks() && w + genphi::hist_row_pairs(n, h.order[static_cast<size_t>(h.begin[static_cast<size_t>(c) + 1])]) >= limit) forced = true;
            sum += w;
        }
        expect(sum == pairs, "the chunks add up", n, sum, pairs);
        expect(forced || h.n_chunks() <= std::max<int64_t>(want, 1), "no more chunks than asked for unless the limit forces them", n, h.n_chunks(), want);
        expect(h.n_chunks() <= static_cast<int64_t>(h.order.size()), "at most one chunk per row", n);
    }
    // the scratch block of this call, with 65 edges
    const int32_t n_edges = 65;
    const size_t n_label = genphi::hist_label_entries(n, group != nullptr), cells = genphi::hist_cells(n_edges, G);
    const genphi::HistScratch s = genphi::hist_scratch(h.order.size(), static_cast<size_t>(h.n_chunks()), n_label, n_edges, cells);
    expect(n_label == (group ? static_cast<size_t>((n + 3) / 4 * 4) : 0) && cells == static_cast<size_t>(std::max(G, 1)) * std::max(G, 1) * 66, "label entries and cells", n);
    expect(s.order % 256 == 0 && s.begin % 256 == 0 && s.label % 256 == 0 && s.thr % 256 == 0 && s.table % 256 == 0 && s.total % 256 == 0, "256-byte alignment", n);
    expect(s.begin - s.order >= h.order.size() * 4 && s.label - s.begin >= (static_cast<size_t>(h.n_chunks()) + 1) * 4 && s.thr - s.label >= n_label * 4 &&
               s.table - s.thr >= static_cast<size_t>(n_edges) * 4 && s.total - s.table >= cells * 8, "every part fits before the next", n);
    expect(s.total <= h.order.size() * 4 + (static_cast<size_t>(h.n_chunks()) + 1) * 4 + n_label * 4 + static_cast<size_t>(n_edges) * 4 + cells * 8 + 5 * 255, "no more than the parts and their padding", n);
}

float next_up(float f) { return std::nextafter(f, std::numeric_limits<float>::infinity()); }
float next_down(float f) { return std::nextafter(f, -std::numeric_limits<float>::infinity()); }

void check_edge(double e)
{
    ++g_edges;
    const float at = genphi::hist_float_at_or_above(e), ab = genphi::hist_float_above(e);
    float around[7];
    const float mid = static_cast<float>(e);
    around[0] = mid; around[1] = next_up(mid); around[2] = next_down(mid); around[3] = next_up(around[1]); around[4] = next_down(around[2]);
    around[5] = 0.0f; around[6] = std::numeric_limits<float>::max();
    for (const float x : around) {
        if (std::isnan(x) || std::isinf(x)) continue;                  // an entry is finite
        expect((x >= at) == (static_cast<double>(x) >= e), "x >= at_or_above(e) decides as (double)x >= e");
        expect((x >= ab) == (static_cast<double>(x) > e), "x >= above(e) decides as (double)x > e");
    }
}

void check_edges()
{
    const double inf = std::numeric_limits<double>::infinity();
    const double special[] = {0.0, -0.0, inf, -inf, 1e-300, -1e-300, 1e300, -1e300, 3.4028234663852886e38, 3.4028235e38, 3.5e38, 1.401298464324817e-45, 7e-46, 1e-46,
                              0.5, 0.25, 1.0, 0.1, 1.0 / 3.0, 4.9e-324};
    for (const double e : special) check_edge(e);
    std::mt19937_64 rng(20);
    for (int k = 0; k < 4000; ++k) {
        uint32_t bits = static_cast<uint32_t>(rng()) & 0x7fffffffu;
        if ((bits >> 23) == 255) bits &= 0x7f7fffffu;
        float f;
        std::memcpy(&f, &bits, 4);
        const double d = static_cast<double>(f);
        check_edge(d);                                                  // on a Float32
        check_edge(std::nextafter(d, inf));                             // one Float64 step above and below it
        check_edge(std::nextafter(d, -inf));
        check_edge((d + static_cast<double>(next_up(f))) / 2);          // half way to the next Float32
        check_edge(-d);
    }
    // the count over the thresholds is the bin of the Float64 definition
    for (int round = 0; round < 200; ++round) {
        const int n_edges = 2 + static_cast<int>(rng() % 40);
        std::vector<double> e(static_cast<size_t>(n_edges));
        double at = round % 3 == 0 ? 0.0 : std::ldexp(1.0, -30);
        for (int b = 0; b < n_edges; ++b) {
            e[static_cast<size_t>(b)] = at;
            const int kind = static_cast<int>(rng() % 4);
            at = kind == 0 ? std::nextafter(at, inf) : kind == 1 ? at + std::ldexp(1.0, -30) : kind == 2 ? at * 1.5 + 1e-9 : static_cast<double>(next_up(static_cast<float>(at)));
            if (!(at > e[static_cast<size_t>(b)])) at = std::nextafter(e[static_cast<size_t>(b)], inf);
        }
        if (round % 5 == 0) e.front() = -inf;
        if (round % 7 == 0) e.back() = inf;
        const std::vector<float> t = genphi::hist_thresholds(n_edges, e.data());
        for (int b = 0; b + 1 < n_edges; ++b) expect(!(t[static_cast<size_t>(b) + 1] < t[static_cast<size_t>(b)]), "the thresholds do not descend");
        ++g_edges;
        for (int b = 0; b < n_edges; ++b) {
            const float c = std::isinf(e[static_cast<size_t>(b)]) ? 0.0f : static_cast<float>(e[static_cast<size_t>(b)]);
            for (const float x : {c, next_up(c), next_down(c), 0.0f, 0.5f}) {
                if (!(x >= 0) || std::isinf(x)) continue;
                const double xd = static_cast<double>(x);
                int want;                                               // 0: below, n_edges: above, else bin + 1
                if (xd < e.front()) want = 0;
                else if (xd > e.back()) want = n_edges;
                else if (xd == e.back()) want = n_edges - 1;
                else {
                    want = 0;
                    while (want < n_edges && e[static_cast<size_t>(want)] <= xd) ++want;
                }
                expect(genphi::hist_count_at_or_below(t, x) == want, "the count over the thresholds is the bin of the definition", round, b, want);
            }
        }
        const float scale = genphi::hist_guess_scale(n_edges, e.data());
        expect(scale >= 0.0f && std::isfinite(scale), "the guess scale is finite and not negative", round);
    }
}

void check_limits()
{
    for (int G = 1; G <= 256; ++G) {
        const int bins = 16384 / G > 4096 ? 4096 : 16384 / G;
        const size_t lds = genphi::hist_lds_bytes(bins + 1, G);
        expect(lds <= 160 * 1024 && lds >= static_cast<size_t>(G) * (bins + 2) * 4, "the LDS request fits 160 KiB and holds the table", G, bins, static_cast<long long>(lds));
    }
    expect(genphi::hist_lds_bytes(4097, 0) == (4097 + 4098) * 4, "LDS of the ungrouped maximum");
    expect(genphi::kSelectPasses * genphi::kSelectDigitBits == 32 && genphi::kSelectDigits * 16 * 4 <= 64 * 1024, "the select tables fit static LDS");
}

}  // namespace

int main()
{
    const int64_t sizes[] = {1, 2, 3, 64, 65, 1025, 100000, 1500000};
    for (const int64_t n : sizes) {
        const int64_t shards[][2] = {{0, n}, {0, 1}, {n - 1, n}, {n / 3, 2 * n / 3 + 1}, {2 < n ? 2 : n, 2 < n ? 2 : n}, {1, n}};
        for (const auto &sh : shards) {
            if (sh[0] < 0 || sh[1] > n || sh[0] > sh[1]) continue;
            for (int pattern = 0; pattern <= 5; ++pattern) {
                if (n >= 100000 && pattern >= 3 && !(sh[0] == 0 && sh[1] == n)) continue;      // (the large sizes: the full range only)
                for (const int64_t want : {int64_t(1), int64_t(4), int64_t(1024), int64_t(1) << 20}) {
                    check_walk(n, sh[0], sh[1], pattern, want, genphi::kHistChunkPairLimit);
                    if (n <= 1025) check_walk(n, sh[0], sh[1], pattern, want, std::max<int64_t>(n, 2));      // a limit that forces cuts: one row more than fits
                }
            }
        }
    }
    // N = 1,500,000 holds 1.1e12 pairs: with one chunk asked for, the limit alone cuts
    {
        const genphi::HistChunks h = genphi::hist_chunks(1500000, 0, 1500000, nullptr, 0, 1);
        expect(h.n_chunks() >= 524 && h.pairs == int64_t(1500000) * 1499999 / 2, "the 2^31 bound forces at least 524 chunks", h.n_chunks());
    }
    check_edges();
    check_limits();
    std::printf("hist geometry check: %lld checks, %lld walks, %lld edges; %lld violations\n", g_checks, g_walks, g_edges, g_violations);
    return g_violations ? 1 : 0;
}
