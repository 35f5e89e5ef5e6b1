// origin_check.cpp -- the host side of gen.simuOrigins (csrc/origin.h) as a stand-alone program: built by tests/test_origins_host.py
// with g++, plain and under AddressSanitizer + UndefinedBehaviorSanitizer.  origin.h is header-only, and its functions read the sizes
// and the listed rows of a plan alone, so the plans here are lists of random lengths.  Checked: the chunk rule for G = 1 .. 32 with
// chunk_arg around every edge (0, 1, the widest - 1, the widest, the widest + 1, n_labels - 1, n_labels, n_labels + 1, 2^31 - 1), by
// walking every chunk exactly once, the stride odd, the LDS within 163,840 bytes and every dword a lane addresses inside it; the pair
// numbering; the list as a set with its groups on random lists with repeats and -1, against a restatement with std::map, and the
// refusal of conflicting and out-of-range groups; the limits at their edges; origin_sizes against the byte counts restated here.
// Prints one summary line; exit status 1 on any violation.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <map>
#include <vector>

#include "../genlib.jl_amd/csrc/origin.h"

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
void expect(bool ok, const char *what, long long at)
{
    if (ok) return;
    ++violations;
    std::fprintf(stderr, "VIOLATION at %lld: %s\n", at, what);
}

long chunk_cases = 0, chunks_walked = 0;

// One (n_labels, G, chunk_arg): the rule's numbers, and a walk over the chunks: they tile [0, n_labels) from multiples of the width, and
// every dword a lane addresses lies inside the 64 tables.
void check_chunks(int64_t n_labels, int32_t G, int64_t arg)
{
    const genphi::OriginChunks c = genphi::origin_chunks(n_labels, G, arg);
    const long long at = (n_labels * 100 + G) * 10000 + arg % 10000;
    ++chunk_cases;
    int64_t widest = 0;                                                  // restated: the largest LC with 256 ((LC G) | 1) <= 163,840
    while (256 * (((widest + 1) * G) | 1) <= 163840) ++widest;
    expect(widest == genphi::origin_max_chunk(G) && widest >= 19, "the widest chunk", at);
    int64_t want = arg > 0 ? arg : widest;
    if (want > widest) want = widest;
    if (want > n_labels) want = n_labels;
    expect(c.chunk_labels == want && want >= 1, "chunk width", at);
    expect(c.chunks == (n_labels + c.chunk_labels - 1) / c.chunk_labels, "chunk count", at);
    expect(c.stride % 2 == 1 && c.stride == ((c.chunk_labels * G) | 1), "odd stride", at);
    expect(c.lds_bytes == 256u * static_cast<size_t>(c.stride) && c.lds_bytes <= genphi::ORIGIN_LDS_BYTES, "LDS bytes", at);
    expect(63 * static_cast<int64_t>(c.stride) + (c.chunk_labels - 1) * G + (G - 1) < static_cast<int64_t>(c.lds_bytes / 4),
           "the last lane's last dword lies in the tables", at);
    bool seen32[2][32] = {}, seen64[64] = {};
    bool clash = false;
    for (int s = 0; s < 64; ++s) {
        const int b32 = static_cast<int>((static_cast<int64_t>(s) * c.stride) % 32), b64 = static_cast<int>((static_cast<int64_t>(s) * c.stride) % 64);
        clash = clash || seen32[s / 32][b32] || seen64[b64];
        seen32[s / 32][b32] = seen64[b64] = true;
    }
    expect(!clash, "bank conflict", at);
    int64_t covered = 0;
    for (int64_t k = 0; k < c.chunks; ++k) {
        const int64_t l0 = k * c.chunk_labels, l1 = l0 + c.chunk_labels < n_labels ? l0 + c.chunk_labels : n_labels;
        expect(l0 == covered && l1 > l0 && l1 - l0 <= c.chunk_labels, "chunks tile the table", at);
        covered = l1;
        ++chunks_walked;
    }
    expect(covered == n_labels, "coverage", at);
}

}  // namespace

int main()
{
    // ---- the chunk rule ----
    for (int32_t G = 1; G <= 32; ++G) {
        const int64_t widest = genphi::origin_max_chunk(G);
        for (int64_t n : {int64_t(1), int64_t(2), widest - 1, widest, widest + 1, 2 * widest - 1, 2 * widest, 2 * widest + 1, int64_t(14798), int64_t(1000000)})
            for (int64_t arg : {int64_t(0), int64_t(1), int64_t(2), int64_t(7), widest - 1, widest, widest + 1, n - 1, n, n + 1, int64_t(2147483647)}) {
                if (arg < 0 || (n == 1000000 && arg > 0 && arg < 7)) continue;
                check_chunks(n, G, arg);
            }
    }
    check_chunks(2147483647, 1, 0);
    {
        const genphi::OriginChunks one = genphi::origin_chunks(1, 1, 0), a = genphi::origin_chunks(639, 1, 0), b = genphi::origin_chunks(640, 1, 0),
                                    c = genphi::origin_chunks(14798, 7, 0), d = genphi::origin_chunks(100, 32, 0), e = genphi::origin_chunks(100, 32, 5),
                                    f = genphi::origin_chunks(90, 7, 0), g = genphi::origin_chunks(10, 2, 100);
        expect(one.chunks == 1 && one.chunk_labels == 1 && one.stride == 1 && one.lds_bytes == 256, "one label", 1);
        expect(a.chunks == 1 && a.chunk_labels == 639 && a.stride == 639 && a.lds_bytes == 163584, "639 labels in one group", 639);
        expect(b.chunks == 2 && b.chunk_labels == 639, "640 labels in one group", 640);
        expect(c.chunk_labels == 91 && c.chunks == 163 && c.stride == 637 && c.lds_bytes == 163072, "14,798 labels in 7 groups", 14798);
        expect(d.chunk_labels == 19 && d.chunks == 6 && d.stride == 609 && d.lds_bytes == 155904, "32 groups", 32);
        expect(e.chunk_labels == 5 && e.chunks == 20 && e.stride == 161, "forced 5", 5);
        expect(f.chunk_labels == 90 && f.chunks == 1 && f.stride == 631, "cut to the table", 90);
        expect(g.chunk_labels == 10 && g.chunks == 1 && g.stride == 21, "cut to the table from above", 10);
        expect(genphi::origin_default_chunk(7) == genphi::origin_max_chunk(7), "the default is the widest", 7);
    }
    // ---- the pair numbering ----
    for (int64_t G = 1; G <= 32; ++G) {
        int64_t p = 0;
        for (int64_t a = 0; a < G; ++a)
            for (int64_t b = a; b < G; ++b) expect(genphi::origin_pair(a, b, G) == p++, "pairs are numbered row-major over the upper triangle", G * 10000 + a * 100 + b);
        expect(p == genphi::origin_pairs(G), "pair count", G);
    }
    // ---- the list, the limits and the sizes on random plans ----
    long plans = 0, conflicts = 0, ranges = 0, repeats = 0, ungrouped = 0;
    for (long k = 0; k < 20000; ++k) {
        genphi::IdentPlan pl;
        pl.n_live = 2 + below(k % 100 == 0 ? 300000 : 3000);
        pl.n_pro = 1 + below(k % 7 == 0 ? 5000 : 60);
        pl.n_labels = 2 + below(2 * pl.n_live - 1);
        pl.planes = 1;
        while ((int64_t(1) << pl.planes) < pl.n_labels) ++pl.planes;
        pl.fa_row.resize(pl.n_live);
        pl.mo_row.resize(pl.n_live);
        pl.row_id.resize(pl.n_live);
        for (int64_t r = 0; r < pl.n_live; ++r) pl.row_id[r] = 1000 + 3 * r;
        pl.const_side.resize(pl.n_labels);
        pl.pro_row.resize(pl.n_pro);
        const int32_t G = static_cast<int32_t>(1 + below(32));
        const bool no_groups = k % 11 == 0, conflict = k % 5 == 1 && pl.n_pro >= 2 && !no_groups, range = k % 13 == 2 && !no_groups && !conflict;
        const int64_t pool = 1 + below(pl.n_live);                       // a small pool makes repeats
        std::map<int32_t, int32_t> of;                                   // row -> group
        std::vector<int32_t> group(pl.n_pro), first;
        for (int64_t i = 0; i < pl.n_pro; ++i) {
            const int32_t r = static_cast<int32_t>(below(pool));
            pl.pro_row[i] = r;
            if (!of.count(r)) {
                of[r] = no_groups ? 0 : static_cast<int32_t>(below(G + 1)) - 1;
                if (of[r] >= 0) first.push_back(r);
            }
            group[i] = of[r];
        }
        if (conflict) {                                                  // the last entry repeats the first with another group
            pl.pro_row[pl.n_pro - 1] = pl.pro_row[0];
            group[pl.n_pro - 1] = group[0] == G - 1 ? group[0] - 1 : group[0] + 1;
        }
        if (range) group[below(pl.n_pro)] = k % 2 ? G : -2;
        genphi::OriginLists ls;
        int64_t bad = -1;
        const int rc = genphi::origin_lists(ls, pl, no_groups ? nullptr : group.data(), no_groups ? 1 : G, bad);
        ++plans;
        if (conflict) {
            ++conflicts;
            expect(rc == genphi::ORIGIN_LIST_CONFLICT && bad == 1000 + 3 * static_cast<int64_t>(pl.pro_row[0]), "two groups for one ID are refused, with the ID", k);
            continue;
        }
        if (range) {
            ++ranges;
            expect(rc == genphi::ORIGIN_LIST_RANGE && bad >= 0 && bad < pl.n_pro && (group[bad] < -1 || group[bad] >= G), "a group out of range is refused, with its entry", k);
            continue;
        }
        expect(rc == genphi::ORIGIN_LIST_OK, "a consistent list is taken", k);
        const int32_t Gn = no_groups ? 1 : G;
        repeats += static_cast<int64_t>(of.size()) < pl.n_pro;
        ungrouped += first.size() < of.size();
        expect(ls.n == static_cast<int64_t>(first.size()) && ls.rows.size() == first.size() && ls.group.size() == first.size() && ls.index.size() == first.size() &&
                   ls.sizes.size() == static_cast<size_t>(Gn),
               "the distinct grouped rows are counted", k);
        bool sorted = true, same = true;
        std::vector<int64_t> sizes(Gn, 0);
        std::vector<char> hit(first.size(), 0);
        for (size_t j = 0; j < ls.rows.size() && same; ++j) {
            const int32_t i = ls.index[j];
            same = i >= 0 && static_cast<size_t>(i) < first.size() && !hit[i] && first[i] == ls.rows[j] && of[ls.rows[j]] == ls.group[j];
            if (same) hit[i] = 1;
            if (same) ++sizes[ls.group[j]];
            if (j) sorted = sorted && (ls.group[j - 1] < ls.group[j] || (ls.group[j - 1] == ls.group[j] && ls.rows[j - 1] < ls.rows[j]));
        }
        expect(same, "every row with its group and its place of first appearance, once", k);
        expect(sorted, "sorted by group, then row", k);
        expect(sizes == ls.sizes, "group sizes", k);
        const bool by_pro = k % 2 == 0;
        const std::string limit = genphi::origin_limits(ls, pl.n_labels, by_pro);
        expect(limit.empty() == (ls.n >= 1 && !(by_pro && ls.n * pl.n_labels > genphi::ORIGIN_MAX_CELLS)), "limits", k);
        const genphi::OriginSizes z = genphi::origin_sizes(pl, ls, Gn, by_pro);
        const size_t L = static_cast<size_t>(pl.n_labels);
        expect(z.copies == 8 * Gn * L && z.autozygous == z.copies && z.matches == 8 * (static_cast<size_t>(Gn) * (Gn + 1) / 2) * L &&
                   z.by_proband == (by_pro ? 4 * static_cast<size_t>(ls.n) * L : 0),
               "result bytes", k);
        expect(z.lists == static_cast<size_t>(4 * (2 * pl.n_live + pl.n_pro) + 8 * (pl.n_live + pl.n_labels) + 12 * ls.n), "list bytes", k);
        const genphi::IdentSizes iz = genphi::ident_sizes(pl, 1000, false);
        expect(z.pair_rows == static_cast<size_t>(32 * pl.planes * pl.n_live) && z.pair_rows == iz.pair_rows, "row bytes are ident's", k);
        expect(z.fixed() == 2 * z.copies + z.matches + z.by_proband + z.lists && z.panel(3) == 3 * z.pair_rows, "sums", k);
    }
    {   // the limits at their edges
        genphi::OriginLists ls;
        ls.n = 32768;
        ls.sizes = {32767, 1};
        expect(genphi::origin_limits(ls, 10, false).empty(), "32,767 in a group are taken", 0);
        expect(genphi::origin_limits(ls, 65535, true).empty() && !genphi::origin_limits(ls, 65536, true).empty() && genphi::origin_limits(ls, 65536, false).empty(),
               "the cell limit at its edge, only by proband", 0);
        ls.sizes = {1, 32768};
        ls.n = 32769;
        expect(!genphi::origin_limits(ls, 10, false).empty(), "32,768 in a group are refused", 0);
        ls.sizes = {0, 0};
        ls.n = 0;
        expect(!genphi::origin_limits(ls, 10, false).empty(), "nobody in a group is refused", 0);
    }
    std::printf("origin check: %ld chunk cases, %ld chunks walked, %ld plans, %ld conflicts refused, %ld groups out of range refused, %ld lists with repeats, "
                "%ld with ungrouped probands; %ld violations\n",
                chunk_cases, chunks_walked, plans, conflicts, ranges, repeats, ungrouped, violations);
    return violations ? 1 : 0;
}
