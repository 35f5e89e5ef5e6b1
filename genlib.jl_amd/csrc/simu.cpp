// simu.cpp -- host plan of gene dropping (see simu.h): the live set, its levels and the parent rows, O(n_ind).
#include "simu.h"

#include <algorithm>

#include "../../include/genphi.h"
#include "ancestor_sweep.h"

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
    std::vector<int32_t> pro_rank(n_pro);
    std::vector<uint8_t> up(n_ind, 0), down(n_ind, 0);
    for (int64_t k = 0; k < n_pro; ++k) {
        const int32_t r = ranks.find(pro_ids[k]);
        if (r < 0) { err = "KeyError: proband " + std::to_string(pro_ids[k]) + " not found"; return GENPHI_ERR_UNKNOWN_ID; }
        pro_rank[k] = r;
        up[r] = 1;
    }
    h.n_pro = n_pro;
    // ---- (a) downwards from the carriers, a listed ancestor blocks; (b) upwards from the probands ----
    for (int64_t i = 0; i < n_ind; ++i)
        down[i] = state[i] >= 0 ? state[i] >= 1 : ((fa[i] >= 0 && down[fa[i]]) || (mo[i] >= 0 && down[mo[i]]));
    for (int64_t i = n_ind - 1; i >= 0; --i)
        if (up[i]) {
            if (fa[i] >= 0) up[fa[i]] = 1;
            if (mo[i] >= 0) up[mo[i]] = 1;
        }
    // ---- levels (a live individual that is not listed has a live parent: the one it is reached through) ----
    std::vector<int32_t> level(n_ind, -1), row(n_ind, -1);
    int32_t n_levels = 0;
    for (int64_t i = 0; i < n_ind; ++i) {
        if (!(down[i] && up[i])) continue;
        level[i] = state[i] >= 0 ? 0 : 1 + std::max(fa[i] >= 0 ? level[fa[i]] : -1, mo[i] >= 0 ? level[mo[i]] : -1);
        n_levels = std::max(n_levels, level[i] + 1);
        ++h.n_live;
    }
    h.n_levels = n_levels;
    h.level_rows.assign(n_levels, 0);
    for (int64_t i = 0; i < n_ind; ++i)
        if (level[i] >= 0) h.level_rows[level[i]]++;
    h.level_begin.assign(n_levels + 1, 0);
    for (int32_t k = 0; k < n_levels; ++k) h.level_begin[k + 1] = h.level_begin[k] + h.level_rows[k];
    // ---- rows: by level, rank order within a level ----
    {
        std::vector<int64_t> fill(h.level_begin.begin(), h.level_begin.end() - (n_levels ? 1 : 0));
        for (int64_t i = 0; i < n_ind; ++i)
            if (level[i] >= 0) row[i] = static_cast<int32_t>(fill[level[i]]++);
    }
    h.fa_row.assign(h.n_live, -1);
    h.mo_row.assign(h.n_live, -1);
    h.row_id.assign(h.n_live, 0);
    h.state0.assign(n_levels ? h.level_rows[0] : 0, 0);
    for (int64_t i = 0; i < n_ind; ++i) {
        const int32_t r = row[i];
        if (r < 0) continue;
        h.row_id[r] = ind[i];
        if (level[i] == 0) { h.state0[r] = state[i]; continue; }          // its own parents are ignored
        if (fa[i] >= 0) h.fa_row[r] = row[fa[i]];
        if (mo[i] >= 0) h.mo_row[r] = row[mo[i]];
    }
    h.pro_row.resize(n_pro);
    h.pro_pos.resize(n_pro);
    for (int64_t k = 0; k < n_pro; ++k) {
        const int32_t r = pro_rank[k];
        h.pro_row[k] = row[r];
        h.pro_pos[k] = state[r] >= 0 ? -2 - state[r] : row[r];
    }
    return GENPHI_OK;
}

}  // namespace genphi
