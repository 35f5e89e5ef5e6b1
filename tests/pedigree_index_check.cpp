// pedigree_index_check.cpp -- the pedigree index (csrc/pedigree_index.cpp: index_pedigree, find_probands) and the rows-by-level builder and
// panel width of the gene-dropping plans (csrc/drop_plan.h) on random pedigrees, as a stand-alone program: built by
// tests/test_pedigree_index_host.py with g++, plain and under AddressSanitizer + UndefinedBehaviorSanitizer, together with
// pedigree_index.cpp.  Everything is checked against a brute-force restatement here (a std::map of the IDs, a sort of the live set by
// level and rank).  Prints one summary line; exit status 1 on any violation.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../genlib.jl_amd/csrc/drop_plan.h"
#include "../genlib.jl_amd/csrc/pedigree_index.h"
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

// n distinct IDs in random order: scheme 0 = 1..n; 1 = non-negative with the largest at 3n + 1023 (the last direct table); 2 = the same
// with the largest at 3n + 1024 (the first hash map); 3 = far apart, every other one negative
std::vector<int64_t> make_ids(int64_t n, int scheme)
{
    std::vector<int64_t> ids;
    if (scheme == 0) {
        for (int64_t i = 0; i < n; ++i) ids.push_back(i + 1);
    } else if (scheme == 3) {
        for (int64_t i = 0; i < n; ++i) ids.push_back((i % 2 ? -1 : 1) * (1000003 * (i + 1) + 7));
    } else {
        const int64_t hi = 3 * n + (scheme == 1 ? 1023 : 1024);
        std::set<int64_t> s{hi};
        while (static_cast<int64_t>(s.size()) < n) s.insert(1 + below(hi));
        ids.assign(s.begin(), s.end());
    }
    for (int64_t i = n - 1; i > 0; --i) std::swap(ids[i], ids[below(i + 1)]);
    return ids;
}

void check_rows(const genphi::DropRows &h, const std::vector<int32_t> &row, const std::vector<int32_t> &level, const std::vector<int64_t> &ind,
                const std::vector<int32_t> &fa, const std::vector<int32_t> &mo, const std::vector<int32_t> &pro_rank, long ped)
{
    const int64_t n = static_cast<int64_t>(level.size());
    std::vector<std::pair<int32_t, int64_t>> live;                // (level, rank), sorted: the order of the rows
    int32_t n_levels = 0;
    for (int64_t i = 0; i < n; ++i)
        if (level[i] >= 0) { live.push_back({level[i], i}); n_levels = std::max(n_levels, level[i] + 1); }
    std::sort(live.begin(), live.end());
    expect(h.n_live == static_cast<int64_t>(live.size()) && h.n_levels == n_levels && h.n_pro == static_cast<int64_t>(pro_rank.size()), "counts", ped);
    expect(static_cast<int64_t>(row.size()) == n, "one row entry per individual", ped);
    expect(static_cast<int32_t>(h.level_rows.size()) == n_levels && static_cast<int32_t>(h.level_begin.size()) == n_levels + 1 && h.level_begin[0] == 0,
           "sizes of the level lists", ped);
    if (violations) return;
    for (int32_t k = 0; k < n_levels; ++k) {
        int64_t members = 0;
        for (const auto &lr : live) members += lr.first == k;
        expect(h.level_rows[k] == members && h.level_begin[k + 1] == h.level_begin[k] + members, "level_rows / level_begin", ped);
    }
    expect(h.level_begin[n_levels] == h.n_live, "the levels cover the rows", ped);
    expect(h.fa_row.size() == live.size() && h.mo_row.size() == live.size() && h.row_id.size() == live.size() && h.pro_row.size() == pro_rank.size(),
           "sizes of the row lists", ped);
    if (violations) return;
    std::vector<char> taken(live.size(), 0);
    for (size_t r = 0; r < live.size(); ++r) {
        const int64_t i = live[r].second;
        expect(row[i] == static_cast<int32_t>(r), "rows are ordered by (level, rank)", ped);
        if (row[i] < 0 || row[i] >= h.n_live) { expect(false, "row out of range", ped); return; }
        expect(!taken[row[i]], "two individuals share a row", ped);
        taken[row[i]] = 1;
        expect(h.level_begin[level[i]] <= row[i] && row[i] < h.level_begin[level[i] + 1], "a row lies in its level's range", ped);
        expect(h.row_id[row[i]] == ind[i], "row_id", ped);
        expect(h.fa_row[row[i]] == (fa[i] >= 0 ? row[fa[i]] : -1) && h.mo_row[row[i]] == (mo[i] >= 0 ? row[mo[i]] : -1), "parent rows", ped);
        if (fa[i] >= 0 && level[fa[i]] >= 0) expect(row[fa[i]] < h.level_begin[level[i]], "a live father's row lies in an earlier level", ped);
        if (mo[i] >= 0 && level[mo[i]] >= 0) expect(row[mo[i]] < h.level_begin[level[i]], "a live mother's row lies in an earlier level", ped);
    }
    for (int64_t i = 0; i < n; ++i)
        if (level[i] < 0) expect(row[i] == -1, "an individual that is not live has no row", ped);
    for (size_t k = 0; k < pro_rank.size(); ++k) expect(h.pro_row[k] == row[pro_rank[k]], "pro_row", ped);
}

}  // namespace

int main()
{
    long pedigrees = 0, rows = 0, direct = 0, hashed = 0, refusals = 0, nobody = 0, one_level = 0;
    for (long ped = 0; ped < 400; ++ped) {
        const int64_t n = 1 + below(200);
        const int scheme = static_cast<int>(ped % 4);
        const std::vector<int64_t> ind = make_ids(n, scheme);
        std::map<int64_t, int64_t> rank;
        for (int64_t i = 0; i < n; ++i) rank[ind[i]] = i;
        std::vector<int64_t> fa(n, 0), mo(n, 0);
        const int64_t p_founder = ped % 7 == 0 ? 100 : 15;             // (every seventh pedigree: founders only, one level)
        for (int64_t i = 1; i < n; ++i) {
            const int64_t r = below(100);
            if (r < p_founder) continue;
            const int64_t lo = std::max<int64_t>(0, i - 30);
            const int64_t f = lo + below(i - lo), m = lo + below(i - lo);
            if (r < 25) fa[i] = ind[f];
            else if (r < 35) mo[i] = ind[m];
            else if (r < 38) fa[i] = mo[i] = ind[f];
            else { fa[i] = ind[f]; mo[i] = ind[m]; }
        }
        const int64_t n_pro = ped % 11 == 0 ? 0 : 1 + below(10);       // (no probands: nobody is live below)
        std::vector<int64_t> pro(n_pro);
        for (auto &p : pro) p = ind[below(n)];
        std::string err;
        // ---- one defect in every fifth pedigree: the code, and the message names the ID ----
        if (ped % 5 == 4 && n >= 3) {
            std::vector<int64_t> ind2 = ind, fa2 = fa, mo2 = mo, pro2 = pro;
            const int64_t i = 1 + below(n - 2), absent = scheme == 3 ? 5 : 3 * n + 2000;
            int want;
            std::string names;
            switch ((ped / 5) % 5) {
            case 0: ind2[i] = ind[i - 1]; fa2[i] = mo2[i] = 0; want = GENPHI_ERR_DUPLICATE_ID; names = "duplicate individual ID " + std::to_string(ind[i - 1]); break;
            case 1: fa2[i] = ind[i + 1]; want = GENPHI_ERR_ORDER; names = ": father " + std::to_string(ind[i + 1]) + " is unknown or listed after its child"; break;
            case 2: mo2[i] = absent; want = GENPHI_ERR_ORDER; names = ": mother " + std::to_string(absent) + " is unknown or listed after its child"; break;
            case 3: mo2[i] = ind[i]; want = GENPHI_ERR_ORDER; names = "individual " + std::to_string(ind[i]) + ": "; break;
            default: pro2.push_back(absent); want = GENPHI_ERR_UNKNOWN_ID; names = "KeyError: proband " + std::to_string(absent) + " not found"; break;
            }
            // (a duplicate: rows that name the overwritten ID as a parent come later and are not reached, or name a known earlier one)
            genphi::PedigreeIndex px;
            std::vector<int32_t> pr;
            int rc = genphi::index_pedigree(px, n, ind2.data(), fa2.data(), mo2.data(), err);
            if (!rc) rc = genphi::find_probands(pr, px.ranks, static_cast<int64_t>(pro2.size()), pro2.data(), err);
            expect(rc == want, "the code of a defect", ped);
            expect(err.find(names) != std::string::npos, "the message of a defect", ped);
            ++refusals;
        }
        // ---- the index ----
        genphi::PedigreeIndex px;
        const int rc = genphi::index_pedigree(px, n, ind.data(), fa.data(), mo.data(), err);
        expect(rc == GENPHI_OK, "index_pedigree failed", ped);
        if (rc) continue;
        ++pedigrees;
        const int64_t lo_id = *std::min_element(ind.begin(), ind.end()), hi_id = *std::max_element(ind.begin(), ind.end());
        expect(px.ranks.direct == (lo_id >= 0 && hi_id < 3 * n + 1024), "direct table or hash map", ped);
        expect(px.ranks.direct == (scheme <= 1), "the scheme's side of the switch", ped);
        (px.ranks.direct ? direct : hashed)++;
        expect(static_cast<int64_t>(px.fa.size()) == n && static_cast<int64_t>(px.mo.size()) == n, "one parent entry per individual", ped);
        for (int64_t i = 0; i < n; ++i) {
            expect(px.ranks.find(ind[i]) == i, "find(own ID) is the rank", ped);
            expect(px.fa[i] == (fa[i] ? rank[fa[i]] : -1) && px.mo[i] == (mo[i] ? rank[mo[i]] : -1), "parent ranks", ped);
            expect(px.fa[i] < i && px.mo[i] < i, "a parent's rank is below its child's", ped);
        }
        for (int64_t id : {int64_t(0), hi_id + 1, lo_id - 1, int64_t(-1), INT64_MAX, INT64_MIN})
            expect(px.ranks.find(id) == (rank.count(id) ? static_cast<int32_t>(rank[id]) : -1), "find(absent ID) is -1", ped);
        std::vector<int32_t> pro_rank;
        expect(genphi::find_probands(pro_rank, px.ranks, n_pro, pro.data(), err) == GENPHI_OK, "find_probands failed", ped);
        expect(static_cast<int64_t>(pro_rank.size()) == n_pro, "one rank per proband", ped);
        for (int64_t k = 0; k < n_pro; ++k) expect(pro_rank[k] == rank[pro[k]], "proband ranks", ped);
        if (violations) break;
        // ---- rows by level: the live set of gen.simuIdentity (the probands and their ancestors), or a random set under its own levels ----
        std::vector<int32_t> level(n, -1);
        std::vector<char> live(n, 0);
        if (ped % 2) {
            for (int32_t r : pro_rank) live[r] = 1;
            for (int64_t i = n - 1; i >= 0; --i)
                if (live[i]) {
                    if (px.fa[i] >= 0) live[px.fa[i]] = 1;
                    if (px.mo[i] >= 0) live[px.mo[i]] = 1;
                }
        } else if (n_pro) {
            for (int64_t i = 0; i < n; ++i) live[i] = below(3) != 0;
        }
        bool any = false;
        for (int64_t i = 0; i < n; ++i) {
            if (!live[i]) continue;
            any = true;
            level[i] = 1 + std::max(px.fa[i] >= 0 ? level[px.fa[i]] : -1, px.mo[i] >= 0 ? level[px.mo[i]] : -1);
        }
        genphi::DropRows h;
        h.n_live = 77; h.n_levels = 5; h.fa_row.assign(3, 9);          // (whatever it held before is gone)
        const std::vector<int32_t> row = genphi::drop_rows(h, level, ind.data(), px.fa, px.mo, pro_rank);
        check_rows(h, row, level, ind, px.fa, px.mo, pro_rank, ped);
        if (violations) break;
        rows += h.n_live;
        nobody += !any;
        one_level += h.n_levels == 1;
        expect(any == (h.n_levels > 0), "no level without a live individual", ped);
    }
    // ---- the empty pedigree ----
    {
        genphi::PedigreeIndex px;
        std::string err;
        std::vector<int32_t> pro_rank;
        expect(genphi::index_pedigree(px, 0, nullptr, nullptr, nullptr, err) == GENPHI_OK && px.fa.empty() && px.mo.empty(), "n_ind = 0", -1);
        expect(px.ranks.find(1) == -1 && px.ranks.find(0) == -1, "n_ind = 0 knows nobody", -1);
        expect(genphi::find_probands(pro_rank, px.ranks, 0, nullptr, err) == GENPHI_OK && pro_rank.empty(), "n_ind = 0, no probands", -1);
        const int64_t one = 1;
        expect(genphi::find_probands(pro_rank, px.ranks, 1, &one, err) == GENPHI_ERR_UNKNOWN_ID && err == "KeyError: proband 1 not found", "n_ind = 0, a proband", -1);
        genphi::DropRows h;
        const std::vector<int32_t> row = genphi::drop_rows(h, {}, nullptr, {}, {}, {});
        expect(row.empty() && h.n_live == 0 && h.n_levels == 0 && h.n_pro == 0 && h.level_rows.empty() && h.level_begin == std::vector<int64_t>{0} &&
                   h.fa_row.empty() && h.mo_row.empty() && h.row_id.empty() && h.pro_row.empty(),
               "rows of the empty pedigree", -1);
    }
    // ---- the panel width: what fits of the default, the argument as it is ----
    {
        int64_t Pn = 0;
        expect(genphi::drop_panel_pairs(5000, 0) == 40 && genphi::drop_panel_pairs(5000, 129) == 2 && genphi::drop_panel_pairs(1, 0) == 1, "drop_panel_pairs", -2);
        expect(genphi::drop_panel_fits(Pn, 5000, 0, 4000.0, 100.0) && Pn == 40, "the default fits whole", -2);
        expect(genphi::drop_panel_fits(Pn, 5000, 0, 1050.0, 100.0) && Pn == 10, "the default is cut to the room", -2);
        expect(!genphi::drop_panel_fits(Pn, 5000, 0, 99.0, 100.0) && Pn == 0, "not one pair fits", -2);
        expect(!genphi::drop_panel_fits(Pn, 5000, 0, -1.0, 100.0), "no room at all", -2);
        expect(genphi::drop_panel_fits(Pn, 5000, 1000, 800.0, 100.0) && Pn == 8, "the argument fits", -2);
        expect(!genphi::drop_panel_fits(Pn, 5000, 1000, 799.0, 100.0) && Pn == 8, "the argument is not cut", -2);
    }
    std::printf("pedigree_index_check: %ld pedigrees, %ld rows, %ld direct tables, %ld hash maps, %ld refusals, %ld with nobody live, %ld of one level, %ld violations\n",
                pedigrees, rows, direct, hashed, refusals, nobody, one_level, violations);
    return violations ? 1 : 0;
}
