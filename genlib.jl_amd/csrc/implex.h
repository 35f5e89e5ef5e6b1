// implex.h -- host plan of gen.implex: the union frontier of the listed probands, generation by generation; no HIP here.
//
// U_g = the individuals at exactly g meioses from any listed proband (an individual can be in several U_g).  Rows of the device
// buffers are POSITIONS in U_g, not individuals: step g reads the compact buffer of U_{g-1} and writes the one of U_g, so no row
// is read that the previous step did not write and nothing is cleared between generations.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace genphi {

struct ImplexPlan {
    int64_t n_pro = 0;                       // listed probands (columns)
    int32_t G = 0;                           // 1 + the longest ascent of any listed proband (0 without probands)
    std::vector<int64_t> rows;               // |U_g|, g = 0 .. G - 1
    std::vector<int64_t> row_begin;          // G + 1: U_g owns [row_begin[g], row_begin[g + 1]) of seen_row
    // U_0: one row per distinct proband (first occurrences, in the caller's order); the listed occurrences (columns) of row r
    // are occ_cols[occ_start[r] .. occ_start[r + 1]), ascending
    std::vector<int32_t> occ_start, occ_cols;
    // U_g, g >= 1: the children of row r that are in U_{g-1}, as positions in U_{g-1} (a child whose father is its mother is
    // listed once): child[child_begin[g] + s[r] .. child_begin[g] + s[r + 1]) with s = edge_start + start_begin[g]
    // (rows[g] + 1 entries, local to the generation)
    std::vector<int32_t> edge_start, child;
    std::vector<int64_t> start_begin, child_begin;    // G + 1 each (generation 0 owns nothing)
    // per row: the individual's position in the union of all U_g; ~position in the generation that meets it first
    std::vector<int32_t> seen_row;
    int64_t n_union = 0, peak_rows = 0, sum_rows = 0, sum_edges = 0;
};

// Returns 0 or a GENPHI_ERR_* code (include/genphi.h); message in err.  Validates the pedigree (order, duplicates), the proband
// IDs and the depth (more than max_generations above the probands: GENPHI_ERR_ARG, found without walking any further).
int plan_implex(ImplexPlan &out, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                const int64_t *pro_ids, int32_t max_generations, std::string &err);

}  // namespace genphi
