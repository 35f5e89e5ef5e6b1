// tree.cpp -- genphi_tree_host (include/genphi.h): gen.phiTree's rounds on a host matrix, with the keys of tree_keys.h that the kernels
// of tree.hip use.  It runs the same synchronous rounds -- every row's best edge out of its component, every component's pick, the
// hooks, the flatten -- so it gives the device's list and the device's number of rounds, and the tests that run without a GPU
// exercise the arithmetic through it.  No HIP here.
#include <algorithm>
#include <cstdint>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/genphi.h"
#include "error.h"
#include "tree_keys.h"

namespace {

// the smallest node of x's tree; halves the path on the way, as find_root (union_find.h) does
int32_t root_of(std::vector<int32_t> &parent, int32_t x)
{
    while (parent[x] != x) {
        parent[x] = parent[parent[x]];
        x = parent[x];
    }
    return x;
}

}  // namespace

extern "C" int genphi_tree_host(const float *m, int64_t n, int64_t ld, double floor, int32_t *row, int32_t *col, float *kinship, int64_t *n_edges,
                                int64_t *n_trees, int32_t *rounds)
{
    static const std::string name = "genphi_tree_host";
    if (n < 0 || n > INT32_MAX) return genphi_set_error(GENPHI_ERR_ARG, name + ": n = " + std::to_string(n) + " is outside 0 .. 2^31 - 1");
    if (floor != floor) return genphi_set_error(GENPHI_ERR_ARG, name + ": the floor is NaN");
    if (n < 2) {
        if (n_edges) *n_edges = 0;
        if (n_trees) *n_trees = n;
        if (rounds) *rounds = 0;
        return GENPHI_OK;
    }
    if (!m) return genphi_set_error(GENPHI_ERR_ARG, name + ": the matrix is NULL");
    if (ld < n) return genphi_set_error(GENPHI_ERR_ARG, name + ": the row pitch " + std::to_string(ld) + " is below n = " + std::to_string(n));
    const int32_t N = static_cast<int32_t>(n);
    std::vector<int32_t> comp, parent;
    std::vector<uint64_t> row_key, pick, edge_pair;
    std::vector<uint32_t> level, edge_bits;
    std::vector<uint8_t> done;
    std::vector<int64_t> order;
    try {
        comp.resize(n);
        parent.resize(n);
        row_key.assign(n, genphi::kTreeNoKey);
        pick.assign(n, genphi::kTreeNoPair);
        level.assign(n, genphi::kTreeNoLevel);
        done.assign(n, 0);
        edge_pair.reserve(n - 1);
        edge_bits.reserve(n - 1);
        order.reserve(n - 1);
    } catch (const std::bad_alloc &) {
        return genphi_set_error(GENPHI_ERR_ALLOC, name + ": no host memory for " + std::to_string(n) + " probands");
    }
    std::iota(comp.begin(), comp.end(), 0);
    std::iota(parent.begin(), parent.end(), 0);
    int32_t done_rounds = 0;
    for (;;) {
        if (done_rounds >= genphi::kTreeMaxRounds)
            return genphi_set_error(GENPHI_ERR_DEVICE, name + ": " + std::to_string(done_rounds) + " rounds did not finish the forest");
        for (int32_t i = 0; i < N; ++i) {               // the rows
            const int32_t ci = comp[i];
            if (done[ci]) continue;
            const float *r = m + static_cast<int64_t>(i) * ld;
            uint64_t best = genphi::kTreeNoKey;
            for (int32_t j = 0; j < N; ++j) {
                if (j == i || comp[j] == ci || !genphi::tree_is_edge(r[j], floor)) continue;
                const uint64_t k = genphi::tree_row_key(genphi::tree_bits(r[j]), j);
                if (k > best) best = k;
            }
            row_key[i] = best;
        }
        for (int32_t i = 0; i < N; ++i)                 // the pick, step 1
            if (row_key[i] != genphi::kTreeNoKey) level[comp[i]] = std::max(level[comp[i]], genphi::tree_level(row_key[i]));
        for (int32_t i = 0; i < N; ++i)                 // ... step 2
            if (row_key[i] != genphi::kTreeNoKey && genphi::tree_level(row_key[i]) == level[comp[i]])
                pick[comp[i]] = std::min(pick[comp[i]], genphi::tree_pair_key(i, genphi::tree_row_key_col(row_key[i])));
        const size_t before = edge_pair.size();
        for (int32_t c = 0; c < N; ++c) {               // the hooks
            if (comp[c] != c || done[c]) continue;
            if (level[c] == genphi::kTreeNoLevel) {
                done[c] = 1;
                continue;
            }
            const int32_t a = comp[genphi::tree_pair_row(pick[c])], b = comp[genphi::tree_pair_col(pick[c])];
            const int32_t other = a == c ? b : a;
            if (!genphi::tree_emits(c, other, pick[c], pick[other])) continue;
            if (static_cast<int64_t>(edge_pair.size()) >= n - 1)
                return genphi_set_error(GENPHI_ERR_DEVICE, name + ": more than " + std::to_string(n - 1) + " edges: is the matrix symmetric?");
            edge_pair.push_back(pick[c]);
            edge_bits.push_back(genphi::tree_level_bits(level[c]));
            const int32_t x = root_of(parent, c), y = root_of(parent, other);
            if (x != y) parent[std::max(x, y)] = std::min(x, y);
        }
        for (int32_t i = 0; i < N; ++i) {               // the flatten
            comp[i] = root_of(parent, i);
            level[i] = genphi::kTreeNoLevel;
            pick[i] = genphi::kTreeNoPair;
        }
        ++done_rounds;
        const size_t emitted = edge_pair.size() - before;
        if (emitted == 0 || static_cast<int64_t>(edge_pair.size()) == n - 1) break;
    }
    const size_t M = edge_pair.size();
    order.resize(M);
    std::iota(order.begin(), order.end(), int64_t{0});
    std::sort(order.begin(), order.end(),
              [&](int64_t x, int64_t y) { return genphi::tree_edge_before(edge_bits[x], edge_pair[x], edge_bits[y], edge_pair[y]); });
    for (size_t k = 0; k < M; ++k) {
        const int64_t o = order[k];
        if (row) row[k] = genphi::tree_pair_row(edge_pair[o]);
        if (col) col[k] = genphi::tree_pair_col(edge_pair[o]);
        if (kinship) kinship[k] = genphi::tree_value(edge_bits[o]);
    }
    if (n_edges) *n_edges = static_cast<int64_t>(M);
    if (n_trees) *n_trees = n - static_cast<int64_t>(M);
    if (rounds) *rounds = done_rounds;
    return GENPHI_OK;
}
