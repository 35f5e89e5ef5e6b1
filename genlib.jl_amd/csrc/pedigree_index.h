// pedigree_index.h -- the index of a pedigree that the host plans of gen.simu, gen.simuIdentity and gen.implex start from: ID -> rank,
// the parents' ranks, the listed probands' ranks, with the planner's rules and messages; no HIP here.
//
// (build_plan in planner.cpp keeps an index of its own: its map grows row by row and, within a row, it checks the parents BEFORE the
// duplicate.  That precedence is behaviour of the gen.phi path and of plan_sweep, which validates through build_plan.)
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

namespace genphi {

// ID -> rank (a direct table for dense non-negative IDs, else a hash map)
struct Ranks {
    std::vector<int32_t> table;
    std::unordered_map<int64_t, int32_t> map;
    bool direct = false;
    void init(int64_t n, const int64_t *ind)             // (here, not in pedigree_index.cpp: plan_sweep needs nothing else of this)
    {
        int64_t lo = INT64_MAX, hi = INT64_MIN;
        for (int64_t i = 0; i < n; ++i) { lo = std::min(lo, ind[i]); hi = std::max(hi, ind[i]); }
        direct = n > 0 && lo >= 0 && hi < 3 * n + 1024;
        if (direct) {
            table.assign(static_cast<size_t>(hi) + 1, -1);
            for (int64_t i = 0; i < n; ++i) table[ind[i]] = static_cast<int32_t>(i);
        } else {
            map.reserve(static_cast<size_t>(n) * 2);
            for (int64_t i = 0; i < n; ++i) map.emplace(ind[i], static_cast<int32_t>(i));
        }
    }
    int32_t find(int64_t id) const
    {
        if (direct) return (id < 0 || id >= static_cast<int64_t>(table.size())) ? -1 : table[id];
        auto it = map.find(id);
        return it == map.end() ? -1 : it->second;
    }
};

struct PedigreeIndex {
    Ranks ranks;
    std::vector<int32_t> fa, mo;             // per rank: the rank of the father / mother, -1 = unknown (ID 0)
};

// Returns 0 or a GENPHI_ERR_* code (include/genphi.h); message in err.  IDs are unique (GENPHI_ERR_DUPLICATE_ID) and parents precede
// their children (GENPHI_ERR_ORDER); the first offending row decides, and within a row the duplicate, then the father, then the mother.
int index_pedigree(PedigreeIndex &out, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, std::string &err);

// The ranks of the listed probands, in list order; GENPHI_ERR_UNKNOWN_ID ("KeyError: proband .. not found") for the first unknown one.
int find_probands(std::vector<int32_t> &pro_rank, const Ranks &ranks, int64_t n_pro, const int64_t *pro_ids, std::string &err);

}  // namespace genphi
