// ident.h -- host plan of gen.simuIdentity (identity coefficients by gene dropping; the definition is the text in
// include/genphi.h): the live set and its levels, the allele table, the parent rows; and what the sweep needs on the device
// as a pure function of the plan.  No HIP here: tests/ident_plan_check.cpp builds it with g++.
//
// The live set L = the listed probands and all their ancestors.  level(x) = 0 when neither parent is known, else 1 + the largest
// level of the known parents.  Rows of the device buffer are POSITIONS in L, ordered by level (rank order within a level).  A
// side whose parent is unknown carries a founder allele: its label is its position in the table of those (ID, side) pairs,
// ascending by ID, then side.  Such a side is constant over the simulations and is written by the init kernel, at any level;
// every other side is written whole by the step of its row's level before anything reads it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "drop_plan.h"

namespace genphi {

struct IdentPlan : DropRows {                // (drop_plan.h: the rows by level; fa_row / mo_row of an unknown parent: -1 - the side's label)
    std::vector<int64_t> allele_id;          // the allele table: the ID ..
    std::vector<int32_t> allele_side;        // .. and the side (0 = from the father) of every label
    std::vector<int64_t> const_side;         // per label: 2 * row + side of the side that carries it
    int64_t n_labels = 0;
    int32_t planes = 1;                      // B = max(1, bit length of n_labels - 1)
};

// Returns 0 or a GENPHI_ERR_* code (include/genphi.h); message in err.  Validates the pedigree (order, duplicates) and the IDs
// as plan_simu does; GENPHI_ERR_ARG for n_labels > 2^31 - 1.  One pass over the pedigree and a sort of the founder sides by ID.
int plan_ident(IdentPlan &out, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
               const int64_t *pro_ids, std::string &err);

// Device bytes of the lists every label sweep uploads (ident.hip, retain.hip, link.hip): the parent rows, the proband rows, the IDs
// and the constant sides.
inline size_t label_list_bytes(const IdentPlan &pl)
{
    return 4 * (pl.fa_row.size() + pl.mo_row.size() + pl.pro_row.size()) + 8 * (pl.row_id.size() + pl.const_side.size());
}

// Device bytes of a sweep (ident.hip allocates exactly these; the check before any launch adds them up).
struct IdentSizes {
    size_t counts = 0;           // Int32 n_pro x n_pro x 9
    size_t labels = 0;           // Int32 n_pro x 2 x S, under GENPHI_IDENT_FLAG_LABELS
    size_t lists = 0;            // the parent rows, the IDs, the constant sides and the proband rows
    size_t pair_rows = 0;        // one pair of words of every live row: 2 sides x B planes x 16 bytes
    size_t pair_gather = 0;      // the same of the listed probands' rows (the pair kernel's dense copy)
    size_t fixed() const { return counts + labels + lists; }
    size_t panel(int64_t pairs) const { return (pair_rows + pair_gather) * static_cast<size_t>(pairs); }
};

inline IdentSizes ident_sizes(const IdentPlan &pl, int64_t S, bool labels)
{
    IdentSizes z;
    const size_t n_pro = static_cast<size_t>(pl.n_pro), side_bytes = 16 * static_cast<size_t>(pl.planes);
    z.counts = 36 * n_pro * n_pro;
    z.labels = labels ? 8 * n_pro * static_cast<size_t>(S) : 0;
    z.lists = label_list_bytes(pl);
    z.pair_rows = 2 * side_bytes * static_cast<size_t>(pl.n_live);
    z.pair_gather = 2 * side_bytes * n_pro;
    return z;
}

}  // namespace genphi
