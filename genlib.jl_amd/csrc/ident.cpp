// ident.cpp -- host plan of gen.simuIdentity (see ident.h): the live set, its levels, the allele table and the parent rows.
#include "ident.h"

#include <algorithm>

#include "../../include/genphi.h"
#include "pedigree_index.h"

namespace genphi {

int plan_ident(IdentPlan &h, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
               const int64_t *pro_ids, std::string &err)
{
    h = IdentPlan();
    PedigreeIndex px;
    if (const int rc = index_pedigree(px, n_ind, ind, father, mother, err)) return rc;
    const std::vector<int32_t> &fa = px.fa, &mo = px.mo;
    // ---- the live set: the listed probands and their ancestors ----
    std::vector<int32_t> pro_rank;
    if (const int rc = find_probands(pro_rank, px.ranks, n_pro, pro_ids, err)) return rc;
    std::vector<uint8_t> live(n_ind, 0);
    for (int32_t r : pro_rank) live[r] = 1;
    for (int64_t i = n_ind - 1; i >= 0; --i)
        if (live[i]) {
            if (fa[i] >= 0) live[fa[i]] = 1;
            if (mo[i] >= 0) live[mo[i]] = 1;
        }
    // ---- levels; rows by level, rank order within a level ----
    std::vector<int32_t> level(n_ind, -1);
    for (int64_t i = 0; i < n_ind; ++i)
        if (live[i]) level[i] = 1 + std::max(fa[i] >= 0 ? level[fa[i]] : -1, mo[i] >= 0 ? level[mo[i]] : -1);
    const std::vector<int32_t> row = drop_rows(h, level, ind, fa, mo, pro_rank);
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
    // ---- the labels: a side with an unknown parent points at its own ----
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
    return GENPHI_OK;
}

}  // namespace genphi
