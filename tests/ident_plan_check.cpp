// ident_plan_check.cpp -- the host plan of gen.simuIdentity (csrc/ident.cpp) on random pedigrees, as a stand-alone program: built by
// tests/test_ident_host.py with g++, plain and under AddressSanitizer + UndefinedBehaviorSanitizer, together with ident.cpp, pedigree_index.cpp and
// ancestor_sweep.cpp.  Every plan is checked against the definition in include/genphi.h, restated here on ranks: the live set by a
// walk from the probands, the levels, the order of the rows, the parent rows, the allele table and its labels, B, the proband rows,
// and the device sizes of ident.h.  Prints one summary line; exit status 1 on any violation.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../genlib.jl_amd/csrc/ident.h"
#include "../include/genphi.h"

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
void expect(bool ok, const char *what, long ped)
{
    if (ok) return;
    ++violations;
    std::fprintf(stderr, "VIOLATION in pedigree %ld: %s\n", ped, what);
}

}  // namespace

int main()
{
    long pedigrees = 0, rows = 0, labels = 0, half_founders = 0, selfings = 0, repeats = 0, refusals = 0;
    int max_planes = 0, max_levels = 0;
    for (long ped = 0; ped < 3000; ++ped) {
        const int64_t n = 1 + below(ped % 50 == 0 ? 1500 : 120);
        const bool sparse_ids = ped % 3 == 0;                   // IDs far apart: the hashed rank table
        std::vector<int64_t> ind(n), fa(n, 0), mo(n, 0);
        for (int64_t i = 0; i < n; ++i) ind[i] = sparse_ids ? 1000003 * (n - i) + 7 : i + 1;      // (descending IDs: the table is re-sorted)
        for (int64_t i = 1; i < n; ++i) {
            const int64_t r = below(100);
            if (r < 15) continue;
            const int64_t lo = std::max<int64_t>(0, i - 30);
            const int64_t f = lo + below(i - lo), m = lo + below(i - lo);
            if (r < 25) fa[i] = ind[f];
            else if (r < 35) mo[i] = ind[m];
            else if (r < 38) fa[i] = mo[i] = ind[f];
            else { fa[i] = ind[f]; mo[i] = ind[m]; }
        }
        const int64_t n_pro = 1 + below(10);
        std::vector<int64_t> pro(n_pro);
        for (auto &p : pro) p = ind[below(n)];
        genphi::IdentPlan pl;
        std::string err;
        const int rc = genphi::plan_ident(pl, n, ind.data(), fa.data(), mo.data(), n_pro, pro.data(), err);
        expect(rc == GENPHI_OK, "plan_ident failed", ped);
        if (rc) continue;
        ++pedigrees;
        // ---- the definition on ranks ----
        std::map<int64_t, int64_t> rank;
        for (int64_t i = 0; i < n; ++i) rank[ind[i]] = i;
        std::vector<int64_t> f(n, -1), m(n, -1), level(n, 0);
        std::vector<char> live(n, 0);
        for (int64_t i = 0; i < n; ++i) {
            if (fa[i]) f[i] = rank[fa[i]];
            if (mo[i]) m[i] = rank[mo[i]];
            level[i] = (f[i] < 0 && m[i] < 0) ? 0 : 1 + std::max(f[i] >= 0 ? level[f[i]] : -1, m[i] >= 0 ? level[m[i]] : -1);
        }
        for (int64_t p : pro) live[rank[p]] = 1;
        for (int64_t i = n - 1; i >= 0; --i)
            if (live[i]) {
                if (f[i] >= 0) live[f[i]] = 1;
                if (m[i] >= 0) live[m[i]] = 1;
            }
        std::vector<std::pair<int64_t, int64_t>> by_level;       // (level, rank) of the live
        std::vector<std::pair<int64_t, int>> table;              // (ID, side)
        for (int64_t i = 0; i < n; ++i) {
            if (!live[i]) continue;
            by_level.emplace_back(level[i], i);
            if (f[i] < 0) table.emplace_back(ind[i], 0);
            if (m[i] < 0) table.emplace_back(ind[i], 1);
            if ((f[i] < 0) != (m[i] < 0)) ++half_founders;
            if (f[i] >= 0 && f[i] == m[i]) ++selfings;
        }
        std::sort(by_level.begin(), by_level.end());
        std::sort(table.begin(), table.end());
        expect(pl.n_pro == n_pro && pl.n_live == static_cast<int64_t>(by_level.size()), "n_live", ped);
        if (pl.n_live != static_cast<int64_t>(by_level.size())) continue;
        std::vector<int64_t> row_of(n, -1);
        std::vector<int64_t> per_level;
        for (size_t r = 0; r < by_level.size(); ++r) {
            row_of[by_level[r].second] = static_cast<int64_t>(r);
            if (static_cast<size_t>(by_level[r].first) >= per_level.size()) per_level.resize(by_level[r].first + 1, 0);
            ++per_level[by_level[r].first];
        }
        expect(pl.n_levels == static_cast<int32_t>(per_level.size()) && pl.level_rows == per_level, "levels", ped);
        expect(pl.level_begin.size() == per_level.size() + 1 && pl.level_begin.back() == pl.n_live && pl.level_begin.front() == 0, "level_begin", ped);
        expect(pl.n_labels == static_cast<int64_t>(table.size()) && pl.n_labels >= 2, "n_labels", ped);
        int planes = 1;
        while ((int64_t(1) << planes) < pl.n_labels) ++planes;
        expect(pl.planes == planes, "planes", ped);
        expect(pl.allele_id.size() == table.size() && pl.allele_side.size() == table.size() && pl.const_side.size() == table.size(), "table sizes", ped);
        if (pl.allele_id.size() != table.size() || pl.const_side.size() != table.size()) continue;
        std::map<std::pair<int64_t, int>, int64_t> label;
        for (size_t k = 0; k < table.size(); ++k) {
            label[table[k]] = static_cast<int64_t>(k);
            expect(pl.allele_id[k] == table[k].first && pl.allele_side[k] == table[k].second, "allele table", ped);
            expect(pl.const_side[k] == 2 * row_of[rank[table[k].first]] + table[k].second, "constant side", ped);
        }
        expect(pl.fa_row.size() == by_level.size() && pl.mo_row.size() == by_level.size() && pl.row_id.size() == by_level.size(), "row lists", ped);
        if (pl.fa_row.size() != by_level.size() || pl.mo_row.size() != by_level.size() || pl.row_id.size() != by_level.size()) continue;
        for (size_t r = 0; r < by_level.size(); ++r) {
            const int64_t i = by_level[r].second;
            expect(pl.row_id[r] == ind[i], "row order", ped);
            const int64_t wf = f[i] >= 0 ? row_of[f[i]] : -1 - label[{ind[i], 0}], wm = m[i] >= 0 ? row_of[m[i]] : -1 - label[{ind[i], 1}];
            expect(pl.fa_row[r] == wf && pl.mo_row[r] == wm, "parent rows", ped);
            expect(f[i] < 0 || row_of[f[i]] < pl.level_begin[by_level[r].first], "father in an earlier level", ped);
            expect(m[i] < 0 || row_of[m[i]] < pl.level_begin[by_level[r].first], "mother in an earlier level", ped);
        }
        std::vector<int64_t> seen(pro);
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) ++repeats;
        for (int64_t k = 0; k < n_pro; ++k) expect(pl.pro_row[k] == row_of[rank[pro[k]]], "proband row", ped);
        const genphi::IdentSizes z = genphi::ident_sizes(pl, 5000, ped % 2 == 0);
        expect(z.counts == static_cast<size_t>(36 * n_pro * n_pro) && z.labels == (ped % 2 == 0 ? static_cast<size_t>(8 * n_pro * 5000) : 0u), "result bytes", ped);
        expect(z.pair_rows == static_cast<size_t>(32 * planes * pl.n_live) && z.pair_gather == static_cast<size_t>(32 * planes * n_pro), "panel bytes", ped);
        expect(z.panel(3) == 3 * (z.pair_rows + z.pair_gather) && z.fixed() == z.counts + z.labels + z.lists, "sums", ped);
        rows += pl.n_live;
        labels += pl.n_labels;
        max_planes = std::max(max_planes, static_cast<int>(pl.planes));
        max_levels = std::max(max_levels, static_cast<int>(pl.n_levels));
        // ---- refusals: an unknown proband, a duplicated ID, a parent after its child ----
        if (ped % 10 == 0) {
            std::vector<int64_t> bad(pro);
            bad.push_back(-5);
            refusals += genphi::plan_ident(pl, n, ind.data(), fa.data(), mo.data(), n_pro + 1, bad.data(), err) == GENPHI_ERR_UNKNOWN_ID;
            if (n >= 2) {
                std::vector<int64_t> dup(ind);
                dup[n - 1] = dup[0];
                refusals += genphi::plan_ident(pl, n, dup.data(), fa.data(), mo.data(), 1, pro.data(), err) == GENPHI_ERR_DUPLICATE_ID;
                std::vector<int64_t> late(fa);
                late[0] = ind[n - 1];
                refusals += genphi::plan_ident(pl, n, ind.data(), late.data(), mo.data(), 1, pro.data(), err) == GENPHI_ERR_ORDER;
            } else {
                refusals += 2;
            }
        }
    }
    expect(genphi::drop_panel_pairs(5000, 0) == 40 && genphi::drop_panel_pairs(5000, 1) == 1 && genphi::drop_panel_pairs(5000, 129) == 2 &&
               genphi::drop_panel_pairs(5000, 1000) == 8 && genphi::drop_panel_pairs(5000, 100000) == 40 && genphi::drop_panel_pairs(1, 0) == 1,
           "panel pairs", -1);
    std::printf("ident plan check: %ld pedigrees, %ld rows, %ld labels, %ld half-founders, %ld selfings, %ld lists with repeats, %ld refusals, "
                "most planes %d, most levels %d; %ld violations\n",
                pedigrees, rows, labels, half_founders, selfings, repeats, refusals, max_planes, max_levels, violations);
    return violations ? 1 : 0;
}
