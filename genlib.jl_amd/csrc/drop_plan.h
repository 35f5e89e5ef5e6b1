// drop_plan.h -- what the two host plans of the four gene-dropping sweeps share (simu.h: simu.hip; ident.h: ident.hip, retain.hip,
// link.hip): the rows of the live set by level, and the width of a panel of simulations.  Host only, no HIP.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace genphi {

// Rows of the device buffer are POSITIONS in the live set, ordered by level (rank order within a level): a step reads rows of any
// earlier level and writes the rows of its own.
struct DropRows {
    int64_t n_pro = 0, n_live = 0;
    int32_t n_levels = 0;                    // 0 when nobody is live
    std::vector<int64_t> level_rows;         // rows per level
    std::vector<int64_t> level_begin;        // n_levels + 1: level k owns the rows [level_begin[k], level_begin[k + 1])
    std::vector<int32_t> fa_row, mo_row;     // per row: the row of the father / mother, -1 = unknown or not live (each plan's own rule on top)
    std::vector<int64_t> row_id;             // per row: the individual's ID (the key of its random stream)
    std::vector<int32_t> pro_row;            // per listed proband: its row, -1 = not live
};

// Fills h from level[i] (-1 = not live; a live individual's level is above those of its live parents), the parents' ranks and the
// probands' ranks.  Returns row[i] per rank (-1 = not live).
inline std::vector<int32_t> drop_rows(DropRows &h, const std::vector<int32_t> &level, const int64_t *ind, const std::vector<int32_t> &fa,
                                      const std::vector<int32_t> &mo, const std::vector<int32_t> &pro_rank)
{
    const int64_t n_ind = static_cast<int64_t>(level.size());
    h = DropRows();
    h.n_pro = static_cast<int64_t>(pro_rank.size());
    for (int64_t i = 0; i < n_ind; ++i) h.n_levels = std::max(h.n_levels, level[i] + 1);
    h.level_rows.assign(h.n_levels, 0);
    for (int64_t i = 0; i < n_ind; ++i)
        if (level[i] >= 0) { h.level_rows[level[i]]++; ++h.n_live; }
    h.level_begin.assign(h.n_levels + 1, 0);
    for (int32_t k = 0; k < h.n_levels; ++k) h.level_begin[k + 1] = h.level_begin[k] + h.level_rows[k];
    std::vector<int32_t> row(n_ind, -1);
    std::vector<int64_t> fill(h.level_begin.begin(), h.level_begin.end() - 1);
    for (int64_t i = 0; i < n_ind; ++i)
        if (level[i] >= 0) row[i] = static_cast<int32_t>(fill[level[i]]++);
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
    h.pro_row.resize(pro_rank.size());
    for (size_t k = 0; k < pro_rank.size(); ++k) h.pro_row[k] = row[pro_rank[k]];
    return row;
}

// The panel width in pairs of words (128 columns): panel_arg rounded up to 128 and cut to S; 0 = all of S.
inline int64_t drop_panel_pairs(int64_t S, int64_t panel_arg)
{
    const int64_t total = (S + 127) / 128;
    return panel_arg > 0 ? std::min(total, (panel_arg + 127) / 128) : total;
}

// Pn = the width above, the default (panel_arg = 0) cut to what room bytes hold at pair_bytes per pair of words.  False: it does not
// fit (GENPHI_ERR_ALLOC with the caller's text; Pn is what did not).
inline bool drop_panel_fits(int64_t &Pn, int64_t S, int64_t panel_arg, double room, double pair_bytes)
{
    Pn = drop_panel_pairs(S, panel_arg);
    if (panel_arg <= 0 && pair_bytes * static_cast<double>(Pn) > room) Pn = static_cast<int64_t>(room / pair_bytes);
    return !(Pn < 1 || room < 0.0 || pair_bytes * static_cast<double>(Pn) > room);
}

}  // namespace genphi
