// simu.cpp -- host plan of gene dropping (see simu.h): the live set, its levels and the parent rows, O(n_ind).
#include "simu.h"

#include <algorithm>

#include "../../include/genphi.h"
#include "pedigree_index.h"

namespace genphi {

int plan_simu(SimuPlan &h, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
              const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, const int32_t *anc_states, std::string &err)
{
    h = SimuPlan();
    for (int64_t k = 0; k < n_anc; ++k)
        if (anc_states[k] < 0 || anc_states[k] > 2) {
            err = "gen.simu: state " + std::to_string(anc_states[k]) + " of ancestor " + std::to_string(anc_ids[k]) + " is outside 0..2";
            return GENPHI_ERR_ARG;
        }
    PedigreeIndex px;
    if (const int rc = index_pedigree(px, n_ind, ind, father, mother, err)) return rc;
    const Ranks &ranks = px.ranks;
    const std::vector<int32_t> &fa = px.fa, &mo = px.mo;
    // ---- the listed ancestors and probands ----
    std::vector<int8_t> state(n_ind, -1);            // -1 = not listed
    for (int64_t k = 0; k < n_anc; ++k) {
        const int32_t r = ranks.find(anc_ids[k]);
        if (r < 0) { err = "KeyError: ancestor " + std::to_string(anc_ids[k]) + " not found"; return GENPHI_ERR_UNKNOWN_ID; }
        if (state[r] >= 0 && state[r] != anc_states[k]) {
            err = "gen.simu: ancestor " + std::to_string(anc_ids[k]) + " is listed with the states " + std::to_string(state[r]) + " and " +
                  std::to_string(anc_states[k]);
            return GENPHI_ERR_ARG;
        }
        state[r] = static_cast<int8_t>(anc_states[k]);
    }
    std::vector<int32_t> pro_rank;
    if (const int rc = find_probands(pro_rank, ranks, n_pro, pro_ids, err)) return rc;
    std::vector<uint8_t> up(n_ind, 0), down(n_ind, 0);
    for (int32_t r : pro_rank) up[r] = 1;
    // ---- (a) downwards from the carriers, a listed ancestor blocks; (b) upwards from the probands ----
    for (int64_t i = 0; i < n_ind; ++i)
        down[i] = state[i] >= 0 ? state[i] >= 1 : ((fa[i] >= 0 && down[fa[i]]) || (mo[i] >= 0 && down[mo[i]]));
    for (int64_t i = n_ind - 1; i >= 0; --i)
        if (up[i]) {
            if (fa[i] >= 0) up[fa[i]] = 1;
            if (mo[i] >= 0) up[mo[i]] = 1;
        }
    // ---- levels (a live individual that is not listed has a live parent: the one it is reached through) ----
    std::vector<int32_t> level(n_ind, -1);
    for (int64_t i = 0; i < n_ind; ++i)
        if (down[i] && up[i]) level[i] = state[i] >= 0 ? 0 : 1 + std::max(fa[i] >= 0 ? level[fa[i]] : -1, mo[i] >= 0 ? level[mo[i]] : -1);
    const std::vector<int32_t> row = drop_rows(h, level, ind, fa, mo, pro_rank);
    // ---- level 0: the listed ancestors; their own parents are ignored ----
    const int64_t n0 = h.n_levels ? h.level_rows[0] : 0;
    std::fill(h.fa_row.begin(), h.fa_row.begin() + n0, -1);
    std::fill(h.mo_row.begin(), h.mo_row.begin() + n0, -1);
    h.state0.assign(n0, 0);
    for (int64_t i = 0; i < n_ind; ++i)
        if (level[i] == 0) h.state0[row[i]] = state[i];
    h.pro_pos.resize(n_pro);
    for (int64_t k = 0; k < n_pro; ++k) {
        const int32_t r = pro_rank[k];
        h.pro_pos[k] = state[r] >= 0 ? -2 - state[r] : row[r];
    }
    return GENPHI_OK;
}

}  // namespace genphi
