// ident.cpp -- host plan of gen.simuIdentity (see ident.h): the live set, its levels, the allele table and the parent rows.
#include "ident.h"

#include <algorithm>

#include "../../include/genphi.h"
#include "ancestor_sweep.h"

namespace genphi {

int plan_ident(IdentPlan &h, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
               const int64_t *pro_ids, std::string &err)
{
    h = IdentPlan();
    // ---- id -> rank; parents must precede their children, IDs are unique (the planner's rules and messages) ----
    Ranks ranks;
    ranks.init(n_ind, ind);
    std::vector<int32_t> fa(n_ind, -1), mo(n_ind, -1);
    for (int64_t i = 0; i < n_ind; ++i) {
        if (ranks.find(ind[i]) != i) { err = "duplicate individual ID " + std::to_string(ind[i]); return GENPHI_ERR_DUPLICATE_ID; }
        if (father[i] != 0) {
            fa[i] = ranks.find(father[i]);
            if (fa[i] < 0 || fa[i] >= i) {
                err = "individual " + std::to_string(ind[i]) + ": father " + std::to_string(father[i]) +
                      " is unknown or listed after its child (pedigree must be in rank order)";
                return GENPHI_ERR_ORDER;
            }
        }
        if (mother[i] != 0) {
            mo[i] = ranks.find(mother[i]);
            if (mo[i] < 0 || mo[i] >= i) {
                err = "individual " + std::to_string(ind[i]) + ": mother " + std::to_string(mother[i]) +
                      " is unknown or listed after its child (pedigree must be in rank order)";
                return GENPHI_ERR_ORDER;
            }
        }
    }
    // ---- the live set: the listed probands and their ancestors ----
    std::vector<int32_t> pro_rank(n_pro);
    std::vector<uint8_t> live(n_ind, 0);
    for (int64_t k = 0; k < n_pro; ++k) {
        const int32_t r = ranks.find(pro_ids[k]);
        if (r < 0) { err = "KeyError: proband " + std::to_string(pro_ids[k]) + " not found"; return GENPHI_ERR_UNKNOWN_ID; }
        pro_rank[k] = r;
        live[r] = 1;
    }
    h.n_pro = n_pro;
    for (int64_t i = n_ind - 1; i >= 0; --i)
        if (live[i]) {
            if (fa[i] >= 0) live[fa[i]] = 1;
            if (mo[i] >= 0) live[mo[i]] = 1;
        }
    // ---- levels; rows by level, rank order within a level ----
    std::vector<int32_t> level(n_ind, -1), row(n_ind, -1);
    int32_t n_levels = 0;
    for (int64_t i = 0; i < n_ind; ++i) {
        if (!live[i]) continue;
        level[i] = 1 + std::max(fa[i] >= 0 ? level[fa[i]] : -1, mo[i] >= 0 ? level[mo[i]] : -1);
        n_levels = std::max(n_levels, level[i] + 1);
        ++h.n_live;
    }
    h.n_levels = n_levels;
    h.level_rows.assign(n_levels, 0);
    for (int64_t i = 0; i < n_ind; ++i)
        if (live[i]) h.level_rows[level[i]]++;
    h.level_begin.assign(n_levels + 1, 0);
    for (int32_t k = 0; k < n_levels; ++k) h.level_begin[k + 1] = h.level_begin[k] + h.level_rows[k];
    {
        std::vector<int64_t> fill(h.level_begin.begin(), h.level_begin.end() - (n_levels ? 1 : 0));
        for (int64_t i = 0; i < n_ind; ++i)
            if (live[i]) row[i] = static_cast<int32_t>(fill[level[i]]++);
    }
    // ---- the allele table: the sides with an unknown parent, ascending by ID, then side ----
    struct Allele {
        int64_t id;
        int32_t side, rank;
    };
    std::vector<Allele> table;
    for (int64_t i = 0; i < n_ind; ++i) {
        if (!live[i]) continue;
        if (fa[i] < 0) table.push_back(Allele{ind[i], 0, static_cast<int32_t>(i)});
        if (mo[i] < 0) table.push_back(Allele{ind[i], 1, static_cast<int32_t>(i)});
    }
    std::sort(table.begin(), table.end(), [](const Allele &a, const Allele &b) { return a.id != b.id ? a.id < b.id : a.side < b.side; });
    h.n_labels = static_cast<int64_t>(table.size());
    if (h.n_labels > INT32_MAX) {
        err = "gen.simuIdentity: " + std::to_string(h.n_labels) + " founder alleles, more than 2^31 - 1";
        return GENPHI_ERR_ARG;
    }
    h.planes = 1;
    while (h.n_labels - 1 >= (int64_t(1) << h.planes)) ++h.planes;
    // ---- the rows ----
    h.fa_row.assign(h.n_live, -1);
    h.mo_row.assign(h.n_live, -1);
    h.row_id.assign(h.n_live, 0);
    for (int64_t i = 0; i < n_ind; ++i) {
        const int32_t r = row[i];
        if (r < 0) continue;
        h.row_id[r] = ind[i];
        if (fa[i] >= 0) h.fa_row[r] = row[fa[i]];
        if (mo[i] >= 0) h.mo_row[r] = row[mo[i]];
    }
    h.allele_id.resize(table.size());
    h.allele_side.resize(table.size());
    h.const_side.resize(table.size());
    for (size_t k = 0; k < table.size(); ++k) {
        const int32_t r = row[table[k].rank];
        h.allele_id[k] = table[k].id;
        h.allele_side[k] = table[k].side;
        h.const_side[k] = 2 * static_cast<int64_t>(r) + table[k].side;
        (table[k].side ? h.mo_row : h.fa_row)[r] = -1 - static_cast<int32_t>(k);
    }
    h.pro_row.resize(n_pro);
    for (int64_t k = 0; k < n_pro; ++k) h.pro_row[k] = row[pro_rank[k]];
    return GENPHI_OK;
}

}  // namespace genphi
