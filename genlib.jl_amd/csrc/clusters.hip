// clusters.hip -- two questions about the graph G_t whose edges are the pairs of probands with kinship >= t, answered from the
// resident result without listing an edge: its connected components (genphi_result_clusters: a lock-free union-find over one read of
// the upper triangle) and a maximal unrelated set (genphi_result_unrelated: the sequential greedy rule, found in rounds over the
// rows).  include/genphi.h states the contract, DESIGN.md 26 the design and the two correctness arguments.  The plan is seen through
// resident.h only; the edge test is over_device.h's, the one genphi_result_over lists by; the union-find is union_find.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/genphi.h"
#include "over_device.h"
#include "resident.h"
#include "resident_graph.h"
#include "union_find.h"

using genphi::al256;
using genphi::device_error;
using genphi::find_root;
using genphi::kOverTile;
using genphi::need_full_f32;
using genphi::over_hits;
using genphi::over_row_hits;
using genphi::parent_of;
using genphi::ResidentView;
using genphi::scratch_for;
using genphi::unite;

namespace {

__global__ __launch_bounds__(256) void cluster_init_kernel(int *parent, int *row_count, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) { parent[i] = i; row_count[i] = 0; }
}

// Workgroup (x, y) walks slab y of row i = row0 + x: slab_cols columns (a multiple of the tile) of the columns right of the diagonal,
// counted from the quad that holds column i + 1, as over_count_kernel walks them; the main launch has one slab, the whole row.  Every
// hit (i, j) is a union.  The row's own root is looked up at the first hit and carried from hit to hit (a union returns it; an
// outdated one is still a node of i's tree, and only sends more hits through unite).  A hit whose column already points at it
// costs one load and no write, which is every hit of a dense threshold once the trees are flat.  row_count[i] += the hits.
__global__ __launch_bounds__(256) void cluster_union_kernel(const float *__restrict__ m, long long ld, int n, double t, int row0, long long slab_cols,
                                                            int *parent, int *row_count)
{
    __shared__ int part[4];
    const int i = row0 + blockIdx.x;
    const long long lo = ((i + 1) & ~3) + (long long)blockIdx.y * slab_cols;
    if (lo >= n) return;                                // (the whole workgroup) the row ends before this slab
    const int end = static_cast<int>(min((long long)n, lo + slab_cols));
    const float *row = m + (long long)i * ld;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    int cnt = 0, ri = -1;
    int jq = static_cast<int>(lo) + (int)threadIdx.x * 4;
    float4 v = zero;
    if (jq < end) v = *reinterpret_cast<const float4 *>(row + jq);
    for (; jq < end; jq += kOverTile) {
        float4 nxt = zero;
        if (jq + kOverTile < end) nxt = *reinterpret_cast<const float4 *>(row + jq + kOverTile);   // in flight across the unions
        unsigned hits = over_hits(v, jq, i, n, t);
        cnt += __popc(hits);
        if (hits && ri < 0) ri = find_root(parent, i);
        while (hits) {
            const int j = jq + __ffs(hits) - 1;
            hits &= hits - 1;
            if (parent_of(parent, j) != ri) ri = unite(parent, ri, j);
        }
        v = nxt;
    }
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_down(cnt, s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int c = part[0] + part[1] + part[2] + part[3];
        if (c) atomicAdd(row_count + i, c);             // (integer adds of the slabs of a row: any order gives the same count)
    }
}

// parent[i] becomes the root of i (in place: a root is an ancestor like any other).  totals != NULL: [0] += the hits of all rows,
// [1] += the roots.  Integer adds: the totals do not depend on who comes first.
__global__ __launch_bounds__(256) void cluster_flatten_kernel(int *parent, int n, const int *row_count, unsigned long long *totals)
{
    __shared__ unsigned long long part[2][4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned long long pairs = 0, roots = 0;
    if (i < n) {
        const int r = find_root(parent, i);
        if (r != i) atomicMin(parent + i, r);
        else roots = 1;
        if (totals) pairs = static_cast<unsigned long long>(row_count[i]);
    }
    if (!totals) return;                                // (the whole grid)
    for (int s = 32; s > 0; s >>= 1) { pairs += __shfl_down(pairs, s); roots += __shfl_down(roots, s); }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = pairs; part[1][threadIdx.x >> 6] = roots; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const unsigned long long x = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
        if (x) atomicAdd(totals + threadIdx.x, x);
    }
}

// The first kSeedRows rows go in a launch of their own, cut into slabs of kSeedSlabTiles tiles so that a few rows still fill the
// machine, and the trees are flattened before the other rows start.  Workgroups that start together all see every node as its own
// root and attempt one compare-and-swap per edge; when the graph is dense that is N^2 / 2 of them on N words.  After the seed rows
// most of a large component hangs under one root, and the rows that follow find their hits joined already.
constexpr int kSeedRows = 16, kSeedSlabTiles = 8;

// ---------------------------------------------------------------------------------------------
// the unrelated set
// ---------------------------------------------------------------------------------------------
constexpr unsigned kUndecided = 0, kIn = 1, kOut = 2;
constexpr int kRowDepth = 4;                            // tiles of a row in flight

// ascending keys = ascending (priority, position): the sign bit flipped makes the unsigned order the signed one
__host__ __device__ __forceinline__ unsigned long long unrelated_key(int priority, int position)
{
    return (static_cast<unsigned long long>(static_cast<unsigned>(priority) ^ 0x80000000u) << 32) | static_cast<unsigned>(position);
}

// degree[i] = the edges at i: one workgroup per row over the whole row but the diagonal, no atomics.  key != NULL: the key of
// (degree[i], i), the order of a call without priorities.
__global__ __launch_bounds__(256) void degree_kernel(const float *__restrict__ m, long long ld, int n, double t, int *__restrict__ degree,
                                                     unsigned long long *__restrict__ key)
{
    __shared__ int part[4];
    const int i = blockIdx.x;
    const float *row = m + (long long)i * ld;
    int cnt = 0;
#pragma unroll 4
    for (int jq = (int)threadIdx.x * 4; jq < n; jq += kOverTile)
        cnt += __popc(over_row_hits(*reinterpret_cast<const float4 *>(row + jq), jq, i, n, t));
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_down(cnt, s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int d = part[0] + part[1] + part[2] + part[3];
        degree[i] = d;
        if (key) key[i] = unrelated_key(d, i);
    }
}

// One round.  The workgroup of a decided row returns before it reads the row.  The workgroup of an undecided row i scans it: i is
// OUT when a neighbour is IN, IN when no undecided neighbour has a smaller key, and waits otherwise.  The states are updated in
// place -- a decision is final and the one the sequential rule makes, so whoever reads it may use it at once, and whoever reads a
// stale UNDECIDED only waits for the next launch.  state: one byte per vertex, read four at a time (the quad's columns; the
// array is padded to a whole quad) by one agent-scope load, written by one agent-scope byte store of its row's workgroup only.
// undecided: the vertices that still wait after this launch.
__global__ __launch_bounds__(256) void unrelated_round_kernel(const float *__restrict__ m, long long ld, int n, double t, unsigned char *state,
                                                              const unsigned long long *__restrict__ key, unsigned long long *undecided)
{
    const int i = blockIdx.x;
    if (__hip_atomic_load(state + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kUndecided) return;     // (the whole workgroup)
    const unsigned long long ki = key[i];
    const float *row = m + (long long)i * ld;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    int blocked = 0, any_in = 0;
    for (int j0 = 0; j0 < n; j0 += kRowDepth * kOverTile) {
        float4 v[kRowDepth];
#pragma unroll
        for (int u = 0; u < kRowDepth; ++u) {
            const int jq = j0 + u * kOverTile + (int)threadIdx.x * 4;
            v[u] = zero;
            if (jq < n) v[u] = *reinterpret_cast<const float4 *>(row + jq);
        }
        int seen_in = 0;
#pragma unroll
        for (int u = 0; u < kRowDepth; ++u) {
            const int jq = j0 + u * kOverTile + (int)threadIdx.x * 4;
            unsigned hits = jq < n ? over_row_hits(v[u], jq, i, n, t) : 0u;
            if (!hits) continue;
            const unsigned s4 = __hip_atomic_load(reinterpret_cast<const unsigned *>(state + jq), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            while (hits) {
                const int e = __ffs(hits) - 1;
                hits &= hits - 1;
                const unsigned s = (s4 >> (8 * e)) & 0xFFu;
                if (s == kIn) seen_in = 1;
                else if (s == kUndecided && key[jq + e] < ki) blocked = 1;
            }
        }
        any_in = __syncthreads_or(seen_in);
        if (any_in) break;                              // (the whole workgroup) the rest of the row cannot change the decision
    }
    const int any_blocked = any_in ? 0 : __syncthreads_or(blocked);
    if (threadIdx.x == 0) {
        if (any_in) __hip_atomic_store(state + i, static_cast<unsigned char>(kOut), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (!any_blocked) __hip_atomic_store(state + i, static_cast<unsigned char>(kIn), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else atomicAdd(undecided, 1ull);
    }
}

}  // namespace

extern "C" {

// gen.phiClusters: parent[i] = i -> one walk of the upper triangle, every hit a union (the first rows ahead of the
// others, with a flatten between) -> flatten and totals -> the labels and 16 bytes of totals come back.  Scratch: the 16 bytes of totals, parent (4 N), the per-row counts (4 N).
int genphi_result_clusters(genphi_plan *p, double threshold, int32_t *label, int64_t *n_clusters, int64_t *n_pairs)
{
    static const char *const name = "genphi_result_clusters";
    if (!p) return genphi_set_error(GENPHI_ERR_ARG, "plan is NULL");
    const ResidentView v = genphi::resident_view(p);
    if (threshold != threshold) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": the threshold is NaN");
    const int64_t N = v.n_pro;
    if (N < 2) {                                        // no pair: every proband is its own cluster
        if (label && N == 1) label[0] = 0;
        if (n_clusters) *n_clusters = N;
        if (n_pairs) *n_pairs = 0;
        return GENPHI_OK;
    }
    int rc = need_full_f32(v, name);
    if (rc) return rc;
    GENPHI_RESIDENT_TRY("hipSetDevice(p->device)", hipSetDevice(v.device));
    const int n = static_cast<int>(N);
    const size_t arr = al256(static_cast<size_t>(N) * sizeof(int));
    char *scratch;
    rc = scratch_for(p, 256 + 2 * arr, name, "the parents and the per-row counts (8 bytes per proband)", &scratch);
    if (rc) return rc;
    unsigned long long *d_tot = reinterpret_cast<unsigned long long *>(scratch);
    int *d_parent = reinterpret_cast<int *>(scratch + 256), *d_cnt = reinterpret_cast<int *>(scratch + 256 + arr);
    const unsigned blocks = static_cast<unsigned>((N + 255) / 256);
    hipError_t e = hipMemsetAsync(d_tot, 0, 16, v.stream);
    if (e == hipSuccess) {
        const long long ld = static_cast<long long>(v.ld);
        hipLaunchKernelGGL(cluster_init_kernel, dim3(blocks), dim3(256), 0, v.stream, d_parent, d_cnt, n);
        int row0 = 0;
        if (n > kSeedRows) {
            const long long slab = static_cast<long long>(kSeedSlabTiles) * kOverTile;
            hipLaunchKernelGGL(cluster_union_kernel, dim3(kSeedRows, static_cast<unsigned>((N + slab - 1) / slab)), dim3(256), 0, v.stream, v.result, ld, n,
                               threshold, 0, slab, d_parent, d_cnt);
            hipLaunchKernelGGL(cluster_flatten_kernel, dim3(blocks), dim3(256), 0, v.stream, d_parent, n, d_cnt, static_cast<unsigned long long *>(nullptr));
            row0 = kSeedRows;
        }
        hipLaunchKernelGGL(cluster_union_kernel, dim3(static_cast<unsigned>(n - row0)), dim3(256), 0, v.stream, v.result, ld, n, threshold, row0,
                           static_cast<long long>(N), d_parent, d_cnt);
        hipLaunchKernelGGL(cluster_flatten_kernel, dim3(blocks), dim3(256), 0, v.stream, d_parent, n, d_cnt, d_tot);
        e = hipGetLastError();
    }
    std::vector<int32_t> h_label;
    unsigned long long h_tot[2] = {0, 0};
    try {
        if (label) h_label.resize(static_cast<size_t>(N));
    } catch (const std::bad_alloc &) {
        (void)hipStreamSynchronize(v.stream);
        return genphi_set_error(GENPHI_ERR_ALLOC, std::string(name) + ": no host memory for the labels");
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_tot, d_tot, sizeof(h_tot), hipMemcpyDeviceToHost, v.stream);
    if (e == hipSuccess && label) e = hipMemcpyAsync(h_label.data(), d_parent, static_cast<size_t>(N) * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream);
    if (e != hipSuccess) return device_error(v, e, name);
    e = hipStreamSynchronize(v.stream);
    if (e != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(name) + ": " + hipGetErrorString(e));
    if (label) std::memcpy(label, h_label.data(), static_cast<size_t>(N) * sizeof(int32_t));      // (outputs are written on success only)
    if (n_clusters) *n_clusters = static_cast<int64_t>(h_tot[1]);
    if (n_pairs) *n_pairs = static_cast<int64_t>(h_tot[0]);
    return GENPHI_OK;
}

// gen.phiUnrelated: the degrees (when they are asked for, or are the priorities) -> keys -> one launch per round
// until the 8-byte count of waiting vertices comes back as zero -> the states and the degrees come back.  Scratch: the count, the
// states (N, padded), the keys (8 N), the degrees (4 N).
int genphi_result_unrelated(genphi_plan *p, double threshold, const int32_t *priority, uint8_t *member, int32_t *degree, int64_t *n_members,
                            int32_t *rounds)
{
    static const char *const name = "genphi_result_unrelated";
    if (!p) return genphi_set_error(GENPHI_ERR_ARG, "plan is NULL");
    const ResidentView v = genphi::resident_view(p);
    if (threshold != threshold) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": the threshold is NaN");
    if (!member) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": member is NULL");
    const int64_t N = v.n_pro;
    if (N < 2) {                                        // no pair: everybody is kept
        if (N == 1) { member[0] = 1; if (degree) degree[0] = 0; }
        if (n_members) *n_members = N;
        if (rounds) *rounds = 0;
        return GENPHI_OK;
    }
    int rc = need_full_f32(v, name);
    if (rc) return rc;
    GENPHI_RESIDENT_TRY("hipSetDevice(p->device)", hipSetDevice(v.device));
    const int n = static_cast<int>(N);
    const size_t state_bytes = al256(static_cast<size_t>(N)), key_bytes = al256(static_cast<size_t>(N) * sizeof(unsigned long long)),
                 deg_bytes = al256(static_cast<size_t>(N) * sizeof(int));
    std::vector<unsigned long long> h_key;
    std::vector<uint8_t> h_state;
    std::vector<int32_t> h_deg;
    try {
        if (priority) {
            h_key.resize(static_cast<size_t>(N));
            for (int64_t i = 0; i < N; ++i) h_key[i] = unrelated_key(priority[i], static_cast<int>(i));
        }
        h_state.resize(static_cast<size_t>(N));
        if (degree) h_deg.resize(static_cast<size_t>(N));
    } catch (const std::bad_alloc &) {
        return genphi_set_error(GENPHI_ERR_ALLOC, std::string(name) + ": no host memory for the keys and the states");
    }
    char *scratch;
    rc = scratch_for(p, 256 + state_bytes + key_bytes + deg_bytes, name, "the states, the keys and the degrees (13 bytes per proband)", &scratch);
    if (rc) return rc;
    unsigned long long *d_wait = reinterpret_cast<unsigned long long *>(scratch);
    unsigned char *d_state = reinterpret_cast<unsigned char *>(scratch + 256);
    unsigned long long *d_key = reinterpret_cast<unsigned long long *>(scratch + 256 + state_bytes);
    int *d_deg = reinterpret_cast<int *>(scratch + 256 + state_bytes + key_bytes);
    const long long ld = static_cast<long long>(v.ld);
    const dim3 grid(static_cast<unsigned>(N));
    static_assert(kUndecided == 0, "the states start from a memset");
    hipError_t e = hipMemsetAsync(d_state, 0, state_bytes, v.stream);
    if (e == hipSuccess && priority) e = hipMemcpyAsync(d_key, h_key.data(), static_cast<size_t>(N) * sizeof(unsigned long long), hipMemcpyHostToDevice, v.stream);
    if (e == hipSuccess && (degree || !priority)) {
        hipLaunchKernelGGL(degree_kernel, grid, dim3(256), 0, v.stream, v.result, ld, n, threshold, d_deg, priority ? nullptr : d_key);
        e = hipGetLastError();
    }
    int32_t launches = 0;
    for (;;) {
        if (e != hipSuccess) return device_error(v, e, name);
        if (launches > n) {                             // the waiting vertex of smallest key decides in every round: never reached
            (void)hipStreamSynchronize(v.stream);
            return genphi_set_error(GENPHI_ERR_DEVICE, std::string(name) + ": " + std::to_string(launches) + " rounds left vertices undecided");
        }
        unsigned long long waiting = 0;
        e = hipMemsetAsync(d_wait, 0, 16, v.stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(unrelated_round_kernel, grid, dim3(256), 0, v.stream, v.result, ld, n, threshold, d_state, d_key, d_wait);
            e = hipGetLastError();
            ++launches;
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&waiting, d_wait, sizeof(waiting), hipMemcpyDeviceToHost, v.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(v.stream);
        if (e != hipSuccess) return device_error(v, e, name);
        if (waiting == 0) break;
    }
    e = hipMemcpyAsync(h_state.data(), d_state, static_cast<size_t>(N), hipMemcpyDeviceToHost, v.stream);
    if (e == hipSuccess && degree) e = hipMemcpyAsync(h_deg.data(), d_deg, static_cast<size_t>(N) * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream);
    if (e != hipSuccess) return device_error(v, e, name);
    e = hipStreamSynchronize(v.stream);
    if (e != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(name) + ": " + hipGetErrorString(e));
    int64_t kept = 0;
    for (int64_t i = 0; i < N; ++i) {                   // (outputs are written on success only)
        member[i] = h_state[i] == kIn ? 1 : 0;
        kept += member[i];
    }
    if (degree) std::memcpy(degree, h_deg.data(), static_cast<size_t>(N) * sizeof(int32_t));
    if (n_members) *n_members = kept;
    if (rounds) *rounds = launches;
    return GENPHI_OK;
}

}  // extern "C"
