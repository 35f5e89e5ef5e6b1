// shard_lists.h -- host-side work lists of a row shard of the result (no HIP here): the continuation of planner.h for a sweep
// that delivers rows [r0, r1) of the proband matrix only (one rank's share of a multi-GPU partition).
#pragma once
#include "planner.h"

namespace genphi {

struct ShardOptions {
    int max_group = 8;                       // children per segment of a hub walk before the step's own limit (walk_lists)
    int max_run = 1;                         // stages per run of a hub walk
    bool no_prune = false;                   // test: the upper levels compute every row
    int force_step = -1, force_row = -1;     // debugging aid: upper step `force_step` computes row `force_row` as well
};

struct ShardLists {
    // the last step: storage row of every proband of the shard and its output row (= proband - r0), in processing order -- the
    // planner's reuse order restricted to the shard; proband order through final_perm when the step is WIDE (it computes every row)
    std::vector<int> rows, out_rows;
    WalkLists last_walk;                     // ... and their hub walk when the step is SPLIT
    // the steps above it, restricted to the rows the shard descends from
    bool pruned = false;                     // false: `upper` is empty, every step runs its own work list
    struct Upper {
        std::vector<int> rows;               // a subsequence of LevelStep::work; empty when the shard needs no row (the launch still writes
                                             // the level's "none" row) and for a WIDE step, which computes and reads every row
        WalkLists walk;                      // SPLIT steps
    };
    std::vector<Upper> upper;                // n_steps - 1 entries
};

// The hub walk of rows of a SPLIT step.  Segments are capped -- the grouping-exact kernel keeps one 32-bit rank mask per child in
// 4 VGPRs, so <= 4 children where it needs them (cut not in rank order), <= 8 where the position test replaces them -- and so are
// runs: a workgroup walks a run's stages one after the other, so one huge run would be a serial tail.
void walk_lists(const LevelStep &s, const int *rows, const int *out_rows, int n_rows, int max_group, int max_run, WalkLists &out);

void build_shard_lists(const Plan &pl, int64_t r0, int64_t r1, const ShardOptions &opt, ShardLists &out);

}  // namespace genphi
