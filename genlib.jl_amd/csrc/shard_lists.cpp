// shard_lists.cpp -- see shard_lists.h
#include "shard_lists.h"

#include <algorithm>
#include <utility>

namespace genphi {

void walk_lists(const LevelStep &s, const int *rows, const int *out_rows, int n_rows, int max_group, int max_run, WalkLists &out)
{
    build_hub_walk(s.srcA.data(), s.srcB.data(), s.ord.data(), static_cast<int32_t>(s.n_prev), rows, out_rows, n_rows,
                   std::min(max_group, s.pos_ord ? 8 : 4), max_run, out);
}

// marks the sources of row i of `s` in the previous cut
static void need_sources(const LevelStep &s, int i, std::vector<char> &need_prev)
{
    if (s.srcA[i] < s.n_prev) need_prev[s.srcA[i]] = 1;
    if (s.srcB[i] < s.n_prev) need_prev[s.srcB[i]] = 1;
}

void build_shard_lists(const Plan &pl, int64_t r0, int64_t r1, const ShardOptions &opt, ShardLists &out)
{
    out = ShardLists();
    const int n_steps = std::max(pl.n_levels - 1, 0);
    const int64_t n_rows = r1 - r0;
    const bool need_perm = !pl.final_perm.empty();
    std::vector<int> &rows = out.rows, &orows = out.out_rows;
    rows.resize(n_rows); orows.resize(n_rows);
    for (int64_t k = 0; k < n_rows; ++k) {
        const int r = static_cast<int>(r0 + k);
        rows[k] = need_perm ? pl.final_perm[r] : r;
        orows[k] = static_cast<int>(k);
    }
    if (n_steps == 0) return;
    const LevelStep &sl = pl.steps[n_steps - 1];
    if (sl.mode != kModeWide) {                  // (a WIDE last step computes every row, in storage order)
        std::vector<int> out_of(sl.n, -1);
        for (int64_t k = 0; k < n_rows; ++k) out_of[rows[k]] = orows[k];
        reuse_order(sl, rows);
        for (int64_t k = 0; k < n_rows; ++k) orows[k] = out_of[rows[k]];
    }
    if (sl.mode == kModeSplit) walk_lists(sl, rows.data(), orows.data(), static_cast<int>(n_rows), opt.max_group, opt.max_run, out.last_walk);

    // upper levels restricted to the ancestors of the shard (walk the sources backwards)
    out.pruned = n_rows < pl.n_pro && n_steps >= 2 && !opt.no_prune;
    if (!out.pruned) return;
    out.upper.resize(n_steps - 1);
    std::vector<char> need(sl.n_prev + 1, 0);    // members of cut n_steps-1
    if (sl.mode == kModeWide) std::fill(need.begin(), need.end(), 1);
    else for (int i : rows) need_sources(sl, i, need);
    for (int st = n_steps - 2; st >= 0; --st) {
        const LevelStep &sv = pl.steps[st];      // produces cut st+1 (n = sv.n)
        std::vector<char> need_prev(sv.n_prev + 1, 0);
        if (opt.force_step == st && opt.force_row >= 0 && opt.force_row < static_cast<int>(need.size())) need[opt.force_row] = 1;
        if (sv.mode == kModeWide)                // computes every row, reads every row
            std::fill(need_prev.begin(), need_prev.end(), 1);
        else {
            std::vector<int> &rw = out.upper[st].rows;
            for (int32_t i : sv.work)            // keep the planner's reuse order
                if (need[i]) { rw.push_back(i); need_sources(sv, i, need_prev); }
            if (sv.mode == kModeSplit) walk_lists(sv, rw.data(), nullptr, static_cast<int>(rw.size()), opt.max_group, opt.max_run, out.upper[st].walk);
        }
        need.swap(need_prev);
    }
}

}  // namespace genphi
