// tree.hip -- genphi_result_tree: the single-linkage tree of the kinships, that is the maximum spanning forest of the graph whose edges
// are the pairs of probands with kinship >= floor, under the strict order of tree_keys.h, found on the resident result by Boruvka's
// rounds.  include/genphi.h states the contract, DESIGN.md 29 the design and the two correctness arguments (the picks of a round form
// a forest; every edge is emitted once).  The plan is seen through resident.h only; the edge test is over_device.h's, the union-find
// union_find.h's, the keys tree_keys.h's, which the host restatement (tree.cpp) shares.
//
// A round is five launches on the view's stream, and a kernel boundary is the only synchronisation between them: within a launch no
// workgroup waits for another.
//   tree_row_kernel      row_key[i] = the best edge that leaves i's component from row i          one read of the active rows
//   tree_level_kernel    level[c] = the largest kinship among the row keys of component c          N entries, integer atomicMax
//   tree_pick_kernel     pick[c] = the smallest (min, max) among the row keys at that kinship      N entries, integer atomicMin
//   tree_hook_kernel     every component with a pick joins the other end's; distinct picks go to the edge buffer
//   tree_flatten_kernel  comp[i] = the root again; level and pick are reset; the round's emitted count goes into its cell
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/genphi.h"
#include "over_device.h"
#include "resident.h"
#include "resident_graph.h"
#include "tree_keys.h"
#include "union_find.h"

using genphi::al256;
using genphi::device_error;
using genphi::find_root;
using genphi::kOverTile;
using genphi::need_full_f32;
using genphi::over_row_hits;
using genphi::ResidentView;
using genphi::scratch_for;
using genphi::unite;

namespace {

// What a call keeps on the device.  comp, level, pick and done are indexed by position; level, pick and done mean something at the
// root of a component only.  comp is written by the flatten kernel alone and read by plain loads in the next launches.
struct TreeState {
    int *comp;                      // the root of i's component at the start of the round (padded to a whole quad)
    int *parent;                    // the union-find the hooks work on
    unsigned long long *row_key;    // tree_row_key of row i's candidate, kTreeNoKey for none
    unsigned *level;                // tree_level of the component's best candidate, kTreeNoLevel for none
    unsigned long long *pick;       // tree_pair_key of the component's pick, kTreeNoPair for none
    unsigned char *done;            // 1: the component found no edge out in some round, it is a finished tree
    unsigned long long *edge_pair;  // the edge buffer: N - 1 slots
    unsigned *edge_bits;
    unsigned long long *cells;      // [0] the edges emitted so far (the slot counter), [1] those of the last round, [2] [0] before it
};

__global__ __launch_bounds__(256) void tree_init_kernel(TreeState s, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    s.comp[i] = i;
    s.parent[i] = i;
    s.row_key[i] = genphi::kTreeNoKey;
    s.level[i] = genphi::kTreeNoLevel;
    s.pick[i] = genphi::kTreeNoPair;
    s.done[i] = 0;
}

// One workgroup per row.  The rows of a finished tree return before they read the matrix (their key is kTreeNoKey since the round
// that finished the tree).  The others read the whole row -- the best edge out of i's component may lead to a column left of i, and
// the full result holds both halves -- test every quad with over_row_hits at `floor`, drop the columns of i's own component, and keep
// the largest tree_row_key.  No atomics: one 8-byte store per row.
__global__ __launch_bounds__(256) void tree_row_kernel(const float *__restrict__ m, long long ld, int n, double floor, TreeState s)
{
    __shared__ unsigned long long part[4];
    const int i = blockIdx.x;
    const int ci = s.comp[i];
    if (s.done[ci]) return;                             // (the whole workgroup)
    const float *row = m + (long long)i * ld;
    unsigned long long best = genphi::kTreeNoKey;
#pragma unroll 4
    for (int jq = (int)threadIdx.x * 4; jq < n; jq += kOverTile) {
        const float4 v = *reinterpret_cast<const float4 *>(row + jq);
        unsigned hits = over_row_hits(v, jq, i, n, floor);
        if (!hits) continue;
        const int4 c = *reinterpret_cast<const int4 *>(s.comp + jq);
        const float x[4] = {v.x, v.y, v.z, v.w};
        const int cj[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (!((hits >> e) & 1u) || cj[e] == ci) continue;
            const unsigned long long k = genphi::tree_row_key(genphi::tree_bits(x[e]), jq + e);
            if (k > best) best = k;
        }
    }
    for (int sh = 32; sh > 0; sh >>= 1) {
        const unsigned long long o = __shfl_down(best, sh);
        if (o > best) best = o;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (part[w] > best) best = part[w];
        s.row_key[i] = best;
    }
}

// level[c] = max over the rows of c.  A row whose level cannot raise the word it reads leaves the atomic out: late rounds have one
// large component, and its rows would otherwise queue on one word.  Integer maxima: the result does not depend on who comes first.
__global__ __launch_bounds__(256) void tree_level_kernel(TreeState s, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = s.row_key[i];
    if (k == genphi::kTreeNoKey) return;
    const unsigned lv = genphi::tree_level(k);
    unsigned *w = s.level + s.comp[i];
    if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < lv) atomicMax(w, lv);
}

// pick[c] = min of tree_pair_key over the rows of c whose candidate attains level[c] (final since the launch before)
__global__ __launch_bounds__(256) void tree_pick_kernel(TreeState s, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = s.row_key[i];
    if (k == genphi::kTreeNoKey) return;
    const int c = s.comp[i];
    if (genphi::tree_level(k) != s.level[c]) return;
    const unsigned long long pr = genphi::tree_pair_key(i, genphi::tree_row_key_col(k));
    unsigned long long *w = s.pick + c;
    if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > pr) atomicMin(w, pr);
}

// One thread per component root.  No pick: the component is a finished tree.  Otherwise it joins the component at the other end of
// its pick (comp is the round's start, untouched here) and emits the edge -- unless the other component picked the same edge and has
// the smaller root (tree_emits): then that one does both.  Slots come from an integer counter; the host's sort removes their order.
__global__ __launch_bounds__(256) void tree_hook_kernel(TreeState s, int n)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n || s.comp[c] != c || s.done[c]) return;
    const unsigned lv = s.level[c];
    if (lv == genphi::kTreeNoLevel) {
        s.done[c] = 1;
        return;
    }
    const unsigned long long pr = s.pick[c];
    if (pr == genphi::kTreeNoPair) return;              // (never: a level comes from a row key, and that row offers its pair)
    const int a = s.comp[genphi::tree_pair_row(pr)], b = s.comp[genphi::tree_pair_col(pr)];
    const int other = a == c ? b : a;
    if (!genphi::tree_emits(c, other, pr, s.pick[other])) return;
    const unsigned long long slot = atomicAdd(s.cells, 1ull);
    if (slot < static_cast<unsigned long long>(n - 1)) {        // (always: the emitted edges form a forest; the host checks the count)
        s.edge_pair[slot] = pr;
        s.edge_bits[slot] = genphi::tree_level_bits(lv);
    }
    unite(s.parent, c, other);
}

__global__ __launch_bounds__(256) void tree_flatten_kernel(TreeState s, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        s.cells[1] = s.cells[0] - s.cells[2];
        s.cells[2] = s.cells[0];
    }
    if (i >= n) return;
    s.comp[i] = find_root(s.parent, i);
    s.level[i] = genphi::kTreeNoLevel;
    s.pick[i] = genphi::kTreeNoPair;
}

}  // namespace

extern "C" {

// gen.phiTree.  Scratch: 256 bytes of cells, then per proband comp (4), parent (4), row_key (8), level (4), pick (8),
// done (1), and the edge buffer's pair (8) and bits (4): 41 bytes per proband.
int genphi_result_tree(genphi_plan *p, double floor, int32_t *row, int32_t *col, float *kinship, int64_t *n_edges, int64_t *n_trees, int32_t *rounds)
{
    static const char *const name = "genphi_result_tree";
    if (!p) return genphi_set_error(GENPHI_ERR_ARG, "plan is NULL");
    const ResidentView v = genphi::resident_view(p);
    if (floor != floor) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": the floor is NaN");
    const int64_t N = v.n_pro;
    if (N < 2) {                                        // no pair: every proband is its own tree
        if (n_edges) *n_edges = 0;
        if (n_trees) *n_trees = N;
        if (rounds) *rounds = 0;
        return GENPHI_OK;
    }
    int rc = need_full_f32(v, name);
    if (rc) return rc;
    GENPHI_RESIDENT_TRY("hipSetDevice(p->device)", hipSetDevice(v.device));
    const int n = static_cast<int>(N);
    const size_t n4 = al256(static_cast<size_t>(N) * 4), n8 = al256(static_cast<size_t>(N) * 8), n1 = al256(static_cast<size_t>(N));
    std::vector<unsigned long long> h_pair;
    std::vector<unsigned> h_bits;
    std::vector<int64_t> order;
    try {
        h_pair.resize(static_cast<size_t>(N - 1));
        h_bits.resize(static_cast<size_t>(N - 1));
        order.reserve(static_cast<size_t>(N - 1));
    } catch (const std::bad_alloc &) {
        return genphi_set_error(GENPHI_ERR_ALLOC, std::string(name) + ": no host memory for the edges");
    }
    char *scratch;
    rc = scratch_for(p, 256 + 4 * n4 + 3 * n8 + n1, name, "the components, the keys and the edge buffer (41 bytes per proband)", &scratch);
    if (rc) return rc;
    TreeState s;
    s.cells = reinterpret_cast<unsigned long long *>(scratch);
    char *at = scratch + 256;
    s.comp = reinterpret_cast<int *>(at);                       at += n4;
    s.parent = reinterpret_cast<int *>(at);                     at += n4;
    s.level = reinterpret_cast<unsigned *>(at);                 at += n4;
    s.edge_bits = reinterpret_cast<unsigned *>(at);             at += n4;
    s.row_key = reinterpret_cast<unsigned long long *>(at);     at += n8;
    s.pick = reinterpret_cast<unsigned long long *>(at);        at += n8;
    s.edge_pair = reinterpret_cast<unsigned long long *>(at);   at += n8;
    s.done = reinterpret_cast<unsigned char *>(at);
    const long long ld = static_cast<long long>(v.ld);
    const dim3 per_entry(static_cast<unsigned>((N + 255) / 256)), per_row(static_cast<unsigned>(N)), wg(256);
    hipError_t e = hipMemsetAsync(s.cells, 0, 256, v.stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(tree_init_kernel, per_entry, wg, 0, v.stream, s, n);
        e = hipGetLastError();
    }
    int32_t done_rounds = 0;
    unsigned long long total = 0;
    for (;;) {
        if (e != hipSuccess) return device_error(v, e, name);
        if (done_rounds >= genphi::kTreeMaxRounds) {    // a round that emits an edge at least halves the growing components: never reached
            (void)hipStreamSynchronize(v.stream);
            return genphi_set_error(GENPHI_ERR_DEVICE, std::string(name) + ": " + std::to_string(done_rounds) + " rounds did not finish the forest");
        }
        hipLaunchKernelGGL(tree_row_kernel, per_row, wg, 0, v.stream, v.result, ld, n, floor, s);
        hipLaunchKernelGGL(tree_level_kernel, per_entry, wg, 0, v.stream, s, n);
        hipLaunchKernelGGL(tree_pick_kernel, per_entry, wg, 0, v.stream, s, n);
        hipLaunchKernelGGL(tree_hook_kernel, per_entry, wg, 0, v.stream, s, n);
        hipLaunchKernelGGL(tree_flatten_kernel, per_entry, wg, 0, v.stream, s, n);
        e = hipGetLastError();
        ++done_rounds;
        unsigned long long emitted = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&emitted, s.cells + 1, sizeof(emitted), hipMemcpyDeviceToHost, v.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(v.stream);
        if (e != hipSuccess) return device_error(v, e, name);
        total += emitted;
        if (total > static_cast<unsigned long long>(N - 1))
            return genphi_set_error(GENPHI_ERR_DEVICE, std::string(name) + ": " + std::to_string(total) + " edges emitted for " + std::to_string(N) + " probands");
        if (emitted == 0 || total == static_cast<unsigned long long>(N - 1)) break;
    }
    const size_t M = static_cast<size_t>(total);
    if (M) {
        e = hipMemcpyAsync(h_pair.data(), s.edge_pair, M * sizeof(unsigned long long), hipMemcpyDeviceToHost, v.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h_bits.data(), s.edge_bits, M * sizeof(unsigned), hipMemcpyDeviceToHost, v.stream);
        if (e != hipSuccess) return device_error(v, e, name);
        e = hipStreamSynchronize(v.stream);
        if (e != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(name) + ": " + hipGetErrorString(e));
    }
    order.resize(M);
    std::iota(order.begin(), order.end(), int64_t{0});
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return genphi::tree_edge_before(h_bits[x], h_pair[x], h_bits[y], h_pair[y]); });
    for (size_t k = 0; k < M; ++k) {                    // (outputs are written on success only)
        const int64_t o = order[k];
        if (row) row[k] = genphi::tree_pair_row(h_pair[o]);
        if (col) col[k] = genphi::tree_pair_col(h_pair[o]);
        if (kinship) kinship[k] = genphi::tree_value(h_bits[o]);
    }
    if (n_edges) *n_edges = static_cast<int64_t>(M);
    if (n_trees) *n_trees = N - static_cast<int64_t>(M);
    if (rounds) *rounds = done_rounds;
    return GENPHI_OK;
}

}  // extern "C"
