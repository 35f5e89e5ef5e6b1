// simu.h -- host plan of gen.simuSample / gen.simuProb (gene dropping): the live set and its levels, top-down; no HIP here.
//
// The live set L = the individuals that (a) are reachable downwards from a listed ancestor of state >= 1 without passing through
// another listed ancestor (the carrier itself included) and (b) are a listed proband or an ancestor of one.  Everyone else has
// zero rows for certain and gets no row.  level(x) = 0 for the listed ancestors in L, else 1 + the largest level of its live
// parents.  Rows of the device buffer are POSITIONS in L, ordered by level (rank order within a level): a step reads rows of any
// earlier level and writes the rows of its own, so nothing but level 0 is ever initialised.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "drop_plan.h"

namespace genphi {

struct SimuPlan : DropRows {                 // (drop_plan.h: the rows by level; fa_row / mo_row of level 0 are -1, its own parents are ignored)
    std::vector<int32_t> state0;             // per row of level 0: the state of the listed ancestor (1 or 2)
    std::vector<int64_t> pro_pos;            // per listed proband: its row, -1 = not live, -2 - state = a listed ancestor of that state
};

// Returns 0 or a GENPHI_ERR_* code (include/genphi.h); message in err.  Validates the pedigree (order, duplicates), the IDs and the
// states (outside 0..2, or an ancestor listed twice with different states: GENPHI_ERR_ARG).  O(n_ind) after one pass.
int plan_simu(SimuPlan &out, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
              const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, const int32_t *anc_states, std::string &err);

}  // namespace genphi
