// hist.hip -- the distribution of the pairwise kinships of the resident result: the histogram over caller-given edges, within and
// between groups of probands (genphi_result_hist), and exact order statistics by radix selection (genphi_result_select).
// include/genphi.h states the contract, DESIGN.md 20 the design, hist_geometry.h the host arithmetic.  The plan is seen through
// resident.h only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/genphi.h"
#include "hist_geometry.h"
#include "resident.h"

using genphi::ResidentView;

// How many rounds of wave aggregation come before the plain LDS atomic (lds_bump4 below): 0 is one atomic per entry.  A
// compile-time choice; profiles/phi_hist_bench.py measures both forms.  The counts do not depend on it.
#ifndef GENPHI_HIST_AGG_ROUNDS
#define GENPHI_HIST_AGG_ROUNDS 2
#endif
// 1: the rounds take one entry of every lane at a time (lds_bump1) instead of its four together.  Measured slower;
// kept selectable for that comparison.
#ifndef GENPHI_HIST_ENTRYWISE
#define GENPHI_HIST_ENTRYWISE 0
#endif

namespace {

constexpr int kThreads = genphi::kHistThreads, kTile = genphi::kHistTile;

// The entry-wise form: one more entry in tab[cell] for every lane with `take`.  A round: the first lane that still waits names its
// cell, a ballot counts the lanes with that cell, that one lane adds the count.
template <int AGG>
__device__ __forceinline__ void lds_bump1(unsigned *tab, int cell, bool take)
{
    if (AGG > 0) {
        const int lane = threadIdx.x & 63;
        unsigned long long left = __ballot(take);
        for (int r = 0; r < AGG; ++r) {
            if (!left) break;                                            // (wave-uniform)
            const int leader = __ffsll(static_cast<long long>(left)) - 1;
            const int c = __builtin_amdgcn_readlane(cell, leader);
            const bool mine = take && cell == c;
            const unsigned long long same = __ballot(mine);
            if (lane == leader) atomicAdd(&tab[c], static_cast<unsigned>(__popcll(same)));
            if (mine) take = false;
            left &= ~same;
        }
    }
    if (take) atomicAdd(&tab[cell], 1u);
}

// One more entry in tab[cell[e]] for every bit e of `take`, for the four entries of every lane of a wave.  Kinship matrices are
// dominated by a handful of values (zeros are often the majority), so most lanes of a wave meet in one counter.  A round: the first
// lane that still waits names the cell c0 .. c3 of its first waiting entry; every lane counts how many of its waiting entries have that
// cell (0 .. 4), three ballots over the bits of those counts give the wave's total, and that one lane adds it.  After AGG rounds
// whatever still waits adds its own 1.  AGG = 0 is one atomic per entry.  Integer adds commute: every form leaves the same counts.
// All 64 lanes of the wave must call this together.
template <int AGG>
__device__ __forceinline__ void lds_bump4(unsigned *tab, int c0, int c1, int c2, int c3, unsigned take)
{
    if (GENPHI_HIST_ENTRYWISE) {
        lds_bump1<AGG>(tab, c0, take & 1u);
        lds_bump1<AGG>(tab, c1, take & 2u);
        lds_bump1<AGG>(tab, c2, take & 4u);
        lds_bump1<AGG>(tab, c3, take & 8u);
        return;
    }
    if (AGG > 0) {
        const int lane = threadIdx.x & 63;
        for (int r = 0; r < AGG; ++r) {
            const unsigned long long waiting = __ballot(take != 0u);
            if (!waiting) break;                                         // (wave-uniform)
            const int leader = __ffsll(static_cast<long long>(waiting)) - 1;
            const int first = (take & 1u) ? c0 : (take & 2u) ? c1 : (take & 4u) ? c2 : c3;
            const int c = __builtin_amdgcn_readlane(first, leader);
            const unsigned hit = ((c0 == c) ? 1u : 0u) | ((c1 == c) ? 2u : 0u) | ((c2 == c) ? 4u : 0u) | ((c3 == c) ? 8u : 0u);
            const unsigned m = __popc(take & hit);
            take &= ~hit;
            const unsigned long long b0 = __ballot(m & 1u), b1 = __ballot(m & 2u), b2 = __ballot(m & 4u);
            if (lane == leader) atomicAdd(&tab[c], static_cast<unsigned>(__popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2)));
        }
    }
    if (take & 1u) atomicAdd(&tab[c0], 1u);
    if (take & 2u) atomicAdd(&tab[c1], 1u);
    if (take & 4u) atomicAdd(&tab[c2], 1u);
    if (take & 8u) atomicAdd(&tab[c3], 1u);
}

// bit e = column jq + e of row i is a pair: right of the diagonal, left of the padding (over_count_kernel's mask)
__device__ __forceinline__ unsigned pair_mask(int jq, int i, int n)
{
    const int lo = min(max(i + 1 - jq, 0), 4), hi = min(max(n - jq, 0), 4);
    return (0xFu << lo) & ~(0xFu << hi) & 0xFu;
}

// The walk both kernels share: the columns right of the diagonal of row i, kWalkDepth tiles of kTile columns at a time, one quad
// per thread and tile, from the quad that holds column i + 1 (16-byte aligned: ld is a multiple of 64).  f(quad, first column,
// mask) is called by every thread of the workgroup the same number of times -- a thread beyond the row passes mask 0 -- so that
// f may ballot.  The loads of the next kWalkDepth tiles are in flight while f works on these: with one tile ahead the walk ran
// at the latency of a load.
constexpr int kWalkDepth = 4;

template <class F>
__device__ __forceinline__ void walk_row(const float *__restrict__ row, int i, int n, F f)
{
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    int jq = ((i + 1) & ~3) + (int)threadIdx.x * 4;
    float4 v[kWalkDepth];
#pragma unroll
    for (int u = 0; u < kWalkDepth; ++u) {
        v[u] = zero;
        if (jq + u * kTile < n) v[u] = *reinterpret_cast<const float4 *>(row + jq + u * kTile);
    }
    for (int j0 = (i + 1) & ~3; j0 < n; j0 += kWalkDepth * kTile, jq += kWalkDepth * kTile) {
        float4 nxt[kWalkDepth];
#pragma unroll
        for (int u = 0; u < kWalkDepth; ++u) {
            nxt[u] = zero;
            const int jn = jq + (kWalkDepth + u) * kTile;
            if (jn < n) nxt[u] = *reinterpret_cast<const float4 *>(row + jn);
        }
#pragma unroll
        for (int u = 0; u < kWalkDepth; ++u) {
            const int ju = jq + u * kTile;
            if (j0 + u * kTile < n) f(v[u], ju, ju < n ? pair_mask(ju, i, n) : 0u);      // (a condition of the whole workgroup)
        }
#pragma unroll
        for (int u = 0; u < kWalkDepth; ++u) v[u] = nxt[u];
    }
}

// every cell that is not zero leaves for out[cell] (64-bit integer atomics: the sum does not depend on who comes first) and is
// zero again
__device__ __forceinline__ void flush(unsigned *tab, int cells, unsigned long long *out)
{
    __syncthreads();
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        const unsigned x = tab[c];
        if (x) {
            atomicAdd(&out[c], static_cast<unsigned long long>(x));
            tab[c] = 0u;
        }
    }
    __syncthreads();
}

struct HistArgs {
    const float *m;                 // the resident rows
    long long ld;
    int n, row_begin;
    const int *order, *begin;       // hist_geometry.h: HistChunks
    const int *label;               // GROUPED: one label per column, -1 padded to a whole quad
    const float *thr;               // hist_thresholds: n_edges of them
    int n_edges, top;               // top: the largest power of two <= n_edges
    float t0, scale;                // thr[0], hist_guess_scale
    int n_groups;                   // max(n_groups, 1)
    unsigned long long *out;        // [row label][column label][n_edges + 1]
};

// k = #{b : thr[b] <= x}, 0 .. n_edges.  The guess is right for (almost) every entry under uniform edges and is believed only
// when thr[g] <= x and not thr[g + 1] <= x, which is the definition of k = g + 1; otherwise the binary search decides.
__device__ __forceinline__ int count_at_or_below(const float *thr, const HistArgs &a, float x)
{
    if (!(x >= a.t0)) return 0;
    const int g = static_cast<int>(fminf((x - a.t0) * a.scale, static_cast<float>(a.n_edges - 1)));    // in [0, n_edges - 1]: x >= t0, scale >= 0
    if (thr[g] <= x && (g + 1 == a.n_edges || !(thr[g + 1] <= x))) return g + 1;
    int k = 0;
    for (int step = a.top; step > 0; step >>= 1) {
        const int j = k + step;
        if (j <= a.n_edges && thr[j - 1] <= x) k = j;
    }
    return k;
}

// A workgroup owns chunk blockIdx.x.  LDS: the thresholds, then the table [column label][n_edges + 1] of the rows of one row
// label; it leaves for the global table when the row label changes and at the end.  A chunk holds fewer than 2^31 pairs, so no
// counter wraps between two flushes.
template <bool GROUPED, int AGG>
__global__ __launch_bounds__(256) void hist_kernel(const HistArgs a)
{
    extern __shared__ unsigned hist_lds[];
    float *thr = reinterpret_cast<float *>(hist_lds);
    unsigned *tab = hist_lds + a.n_edges;
    const int stride = a.n_edges + 1, cells = a.n_groups * stride;
    for (int c = threadIdx.x; c < a.n_edges; c += kThreads) thr[c] = a.thr[c];
    for (int c = threadIdx.x; c < cells; c += kThreads) tab[c] = 0u;
    __syncthreads();
    const int p0 = a.begin[blockIdx.x], p1 = a.begin[blockIdx.x + 1];
    int cur = GROUPED ? a.label[a.order[p0]] : 0;
    for (int p = p0; p < p1; ++p) {
        const int i = a.order[p];
        if (GROUPED) {
            const int g = a.label[i];
            if (g != cur) {                                              // (the whole workgroup)
                flush(tab, cells, a.out + (size_t)cur * cells);
                cur = g;
            }
        }
        walk_row(a.m + (long long)(i - a.row_begin) * a.ld, i, a.n, [&](const float4 v, int jq, unsigned mask) {
            int4 lab = make_int4(0, 0, 0, 0);
            if (GROUPED && mask) lab = *reinterpret_cast<const int4 *>(a.label + jq);           // (jq < n <= the padded length)
            const unsigned take = mask & ((lab.x >= 0 ? 1u : 0u) | (lab.y >= 0 ? 2u : 0u) | (lab.z >= 0 ? 4u : 0u) | (lab.w >= 0 ? 8u : 0u));
            const int c0 = (take & 1u) ? lab.x * stride + count_at_or_below(thr, a, v.x) : 0;
            const int c1 = (take & 2u) ? lab.y * stride + count_at_or_below(thr, a, v.y) : 0;
            const int c2 = (take & 4u) ? lab.z * stride + count_at_or_below(thr, a, v.z) : 0;
            const int c3 = (take & 8u) ? lab.w * stride + count_at_or_below(thr, a, v.w) : 0;
            lds_bump4<AGG>(tab, c0, c1, c2, c3, take);
        });
    }
    flush(tab, cells, a.out + (size_t)cur * cells);
}

struct SelectArgs {
    const float *m;
    long long ld;
    int n, row_begin;
    const int *order, *begin;
    int n_prefix, shift;            // the digit is bits shift .. shift + kSelectDigitBits - 1 of the pattern
    unsigned prefix[GENPHI_SELECT_MAX_RANKS];       // distinct: what the bits above the digit must be
    unsigned long long *out;        // [prefix][digit]
};

// One radix pass: the histogram of one digit of the entries whose higher bits are one of the live prefixes, one LDS table per
// prefix.  The prefixes are distinct, so an entry meets one table at most.
template <int AGG>
__global__ __launch_bounds__(256) void select_kernel(const SelectArgs a)
{
    __shared__ unsigned tab[GENPHI_SELECT_MAX_RANKS * genphi::kSelectDigits];
    const int cells = a.n_prefix * genphi::kSelectDigits;
    for (int c = threadIdx.x; c < cells; c += kThreads) tab[c] = 0u;
    __syncthreads();
    const int p0 = a.begin[blockIdx.x], p1 = a.begin[blockIdx.x + 1];
    for (int p = p0; p < p1; ++p) {
        const int i = a.order[p];
        walk_row(a.m + (long long)(i - a.row_begin) * a.ld, i, a.n, [&](const float4 v, int jq, unsigned mask) {
            (void)jq;
            auto cell_of = [&](float x) {                                    // -1: the higher bits match no live prefix
                const unsigned long long key = __float_as_uint(x);
                const unsigned high = static_cast<unsigned>(key >> (a.shift + genphi::kSelectDigitBits));      // (64-bit: the first pass shifts by 32)
                int slot = -1;
                for (int q = 0; q < a.n_prefix; ++q)
                    if (a.prefix[q] == high) slot = q;
                return slot < 0 ? -1 : slot * genphi::kSelectDigits + static_cast<int>((key >> a.shift) & (genphi::kSelectDigits - 1));
            };
            const int c0 = cell_of(v.x), c1 = cell_of(v.y), c2 = cell_of(v.z), c3 = cell_of(v.w);
            const unsigned take = mask & ((c0 >= 0 ? 1u : 0u) | (c1 >= 0 ? 2u : 0u) | (c2 >= 0 ? 4u : 0u) | (c3 >= 0 ? 8u : 0u));
            lds_bump4<AGG>(tab, c0, c1, c2, c3, take);
        });
    }
    flush(tab, cells, a.out);
}

// not the Float64 result; then *empty for an empty shard (GENPHI_OK), else a resident result with rows
int need_f32_rows(const ResidentView &v, const char *name, bool *empty)
{
    *empty = false;
    if (v.res_f64) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + " works on the Float32 result (gen.phi's matrix)");
    if (v.res_known && v.n_rows == 0) { *empty = true; return GENPHI_OK; }
    if (!v.on_device || !v.result || v.n_rows == 0) return genphi_set_error(GENPHI_ERR_DEVICE, "no resident result: call genphi_compute_device first");
    return GENPHI_OK;
}

int check_pitch(const ResidentView &v, const char *name)
{
    if (v.ld < v.n_pro || v.ld % 64 != 0 || v.n_pro > INT32_MAX || v.row_begin < 0 || v.row_begin + v.n_rows > v.n_pro)
        return genphi_set_error(GENPHI_ERR_DEVICE, std::string(name) + ": unexpected row pitch " + std::to_string(v.ld) + " or row range");
    return GENPHI_OK;
}

int scratch_for(genphi_plan *p, size_t bytes, const char *name, const char *what, char **scratch)
{
    if (genphi::resident_scratch(p, bytes, scratch) == GENPHI_OK) return GENPHI_OK;
    return genphi_set_error(GENPHI_ERR_ALLOC, std::string(name) + ": " + std::to_string(bytes) + " bytes of device memory for " + what + ": " + genphi_last_error());
}

int64_t chunks_wanted(const ResidentView &v) { return static_cast<int64_t>(std::max(v.n_cus, 1)) * genphi::kHistChunksPerCu; }

// the rest of a call after its launch: the table comes back, the stream is synchronised also after an error
int table_back(const ResidentView &v, hipError_t e, std::vector<uint64_t> &host, const void *dev, const char *name)
{
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), dev, host.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, v.stream);
    const hipError_t es = hipStreamSynchronize(v.stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(name) + ": " + hipGetErrorString(e));
    return GENPHI_OK;
}

}  // namespace

extern "C" {

int genphi_result_hist(genphi_plan *p, int32_t n_edges, const double *edges, int32_t n_groups, const int32_t *group, int64_t *counts,
                       int64_t *below, int64_t *above, int64_t *n_pairs)
{
    static const char *const name = "genphi_result_hist";
    if (!p) return genphi_set_error(GENPHI_ERR_ARG, "plan is NULL");
    const ResidentView v = genphi::resident_view(p);
    if (!edges) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": edges is NULL");
    if (n_edges < 2 || n_edges > GENPHI_HIST_MAX_EDGES)
        return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": n_edges = " + std::to_string(n_edges) + " outside [2, " + std::to_string(GENPHI_HIST_MAX_EDGES) + "]");
    for (int32_t b = 0; b < n_edges; ++b) {
        if (edges[b] != edges[b]) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": edge " + std::to_string(b) + " is NaN");
        if (b && !(edges[b - 1] < edges[b]))
            return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": the edges are not strictly increasing at " + std::to_string(b));
    }
    if (group ? (n_groups < 1 || n_groups > GENPHI_HIST_MAX_GROUPS) : (n_groups < 0 || n_groups > 1))
        return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": n_groups = " + std::to_string(n_groups) +
                                                    (group ? " outside [1, " + std::to_string(GENPHI_HIST_MAX_GROUPS) + "]" : " without labels: 0 or 1"));
    const int32_t G = std::max(n_groups, 1), n_bins = n_edges - 1;
    if (static_cast<int64_t>(G) * n_bins > GENPHI_HIST_MAX_CELLS)
        return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": " + std::to_string(G) + " groups x " + std::to_string(n_bins) + " bins exceed " +
                                                    std::to_string(GENPHI_HIST_MAX_CELLS) + " cells");
    const int64_t N = v.n_pro;
    if (group)
        for (int64_t i = 0; i < N; ++i)
            if (group[i] < -1 || group[i] >= n_groups)
                return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": label " + std::to_string(group[i]) + " of proband " + std::to_string(i) +
                                                            " outside [-1, " + std::to_string(n_groups) + ")");
    auto deliver = [&](const std::vector<uint64_t> *tab) {                      // tab: [row label][column label][n_edges + 1], or NULL for zeros
        const size_t stride = static_cast<size_t>(n_edges) + 1;
        int64_t total = 0;
        for (int32_t r = 0; r < G; ++r)
            for (int32_t c = 0; c < G; ++c) {
                const size_t rc = static_cast<size_t>(r) * G + c, cr = static_cast<size_t>(c) * G + r;
                for (size_t k = 0; k < stride; ++k) {
                    const int64_t x = !tab ? 0 : static_cast<int64_t>((*tab)[rc * stride + k] + (r != c ? (*tab)[cr * stride + k] : 0));
                    if (r <= c) total += x;
                    if (k == 0) { if (below) below[rc] = x; }
                    else if (k == stride - 1) { if (above) above[rc] = x; }
                    else if (counts) counts[rc * n_bins + (k - 1)] = x;
                }
            }
        if (n_pairs) *n_pairs = total;
        return GENPHI_OK;
    };
    if (N < 2) return deliver(nullptr);
    bool empty;
    int rc = need_f32_rows(v, name, &empty);
    if (rc) return rc;
    if (empty) return deliver(nullptr);
    rc = check_pitch(v, name);
    if (rc) return rc;
    GENPHI_RESIDENT_TRY("hipSetDevice(p->device)", hipSetDevice(v.device));

    genphi::HistChunks ch;
    std::vector<float> thr;
    std::vector<int32_t> lab;
    std::vector<uint64_t> tab;
    const size_t cells = genphi::hist_cells(n_edges, n_groups);
    try {
        ch = genphi::hist_chunks(N, v.row_begin, v.row_begin + v.n_rows, group, n_groups, chunks_wanted(v));
        thr = genphi::hist_thresholds(n_edges, edges);
        if (group) {
            lab.assign(genphi::hist_label_entries(N, true), -1);
            std::memcpy(lab.data(), group, static_cast<size_t>(N) * sizeof(int32_t));
        }
        tab.assign(cells, 0);
    } catch (const std::bad_alloc &) {
        return genphi_set_error(GENPHI_ERR_ALLOC, std::string(name) + ": no host memory for the tables");
    }
    if (ch.n_chunks() == 0) return deliver(nullptr);                            // no row with a pair, or none with a label
    const genphi::HistScratch s = genphi::hist_scratch(ch.order.size(), static_cast<size_t>(ch.n_chunks()), lab.size(), thr.size(), cells);
    char *scratch;
    rc = scratch_for(p, s.total, name, "the walk order, the edges and the table of counts", &scratch);
    if (rc) return rc;
    HistArgs a;
    a.m = v.result; a.ld = static_cast<long long>(v.ld); a.n = static_cast<int>(N); a.row_begin = static_cast<int>(v.row_begin);
    a.order = reinterpret_cast<const int *>(scratch + s.order); a.begin = reinterpret_cast<const int *>(scratch + s.begin);
    a.label = group ? reinterpret_cast<const int *>(scratch + s.label) : nullptr;
    a.thr = reinterpret_cast<const float *>(scratch + s.thr);
    a.n_edges = n_edges;
    a.top = 1;
    while (a.top * 2 <= n_edges) a.top *= 2;
    a.t0 = thr[0]; a.scale = genphi::hist_guess_scale(n_edges, edges);
    a.n_groups = G;
    a.out = reinterpret_cast<unsigned long long *>(scratch + s.table);
    const size_t lds = genphi::hist_lds_bytes(n_edges, n_groups);
    const void *fn = group ? reinterpret_cast<const void *>(hist_kernel<true, GENPHI_HIST_AGG_ROUNDS>) : reinterpret_cast<const void *>(hist_kernel<false, GENPHI_HIST_AGG_ROUNDS>);
    hipError_t e = lds > 32768 ? hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpyAsync(scratch + s.order, ch.order.data(), ch.order.size() * sizeof(int32_t), hipMemcpyHostToDevice, v.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(scratch + s.begin, ch.begin.data(), ch.begin.size() * sizeof(int32_t), hipMemcpyHostToDevice, v.stream);
    if (e == hipSuccess && group) e = hipMemcpyAsync(scratch + s.label, lab.data(), lab.size() * sizeof(int32_t), hipMemcpyHostToDevice, v.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(scratch + s.thr, thr.data(), thr.size() * sizeof(float), hipMemcpyHostToDevice, v.stream);
    if (e == hipSuccess) e = hipMemsetAsync(scratch + s.table, 0, cells * sizeof(uint64_t), v.stream);
    if (e == hipSuccess) {
        const dim3 grid(static_cast<unsigned>(ch.n_chunks()));
        if (group) hipLaunchKernelGGL((hist_kernel<true, GENPHI_HIST_AGG_ROUNDS>), grid, dim3(kThreads), lds, v.stream, a);
        else hipLaunchKernelGGL((hist_kernel<false, GENPHI_HIST_AGG_ROUNDS>), grid, dim3(kThreads), lds, v.stream, a);
        e = hipGetLastError();
    }
    rc = table_back(v, e, tab, scratch + s.table, name);                        // (the host vectors are read until here)
    if (rc) return rc;
    return deliver(&tab);
}

int genphi_result_select(genphi_plan *p, int32_t n_ranks, const int64_t *ranks, float *values, int64_t *n_pairs)
{
    static const char *const name = "genphi_result_select";
    if (!p) return genphi_set_error(GENPHI_ERR_ARG, "plan is NULL");
    const ResidentView v = genphi::resident_view(p);
    if (n_ranks < 0 || n_ranks > GENPHI_SELECT_MAX_RANKS || (n_ranks == 0 && values))
        return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": n_ranks = " + std::to_string(n_ranks) + " outside [1, " + std::to_string(GENPHI_SELECT_MAX_RANKS) +
                                                    "] (0 with values == NULL only reports *n_pairs)");
    if (n_ranks > 0 && !ranks) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": ranks is NULL");
    if (n_ranks > 0 && !values) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": values is NULL");
    const int64_t N = v.n_pro;
    bool empty = N < 2;
    if (!empty) {
        const int rc = need_f32_rows(v, name, &empty);
        if (rc) return rc;
    }
    if (!empty) {
        const int rc = check_pitch(v, name);
        if (rc) return rc;
    }
    const int64_t total = empty ? 0 : genphi::hist_pairs_of_rows(N, v.row_begin, v.row_begin + v.n_rows);
    for (int32_t r = 0; r < n_ranks; ++r)
        if (ranks[r] < 0 || ranks[r] >= total)
            return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": rank " + std::to_string(ranks[r]) + " outside [0, " + std::to_string(total) + ")");
    if (n_ranks == 0) {
        if (n_pairs) *n_pairs = total;
        return GENPHI_OK;
    }
    GENPHI_RESIDENT_TRY("hipSetDevice(p->device)", hipSetDevice(v.device));

    genphi::HistChunks ch;
    std::vector<uint64_t> tab;
    try {
        ch = genphi::hist_chunks(N, v.row_begin, v.row_begin + v.n_rows, nullptr, 0, chunks_wanted(v));
        tab.reserve(static_cast<size_t>(GENPHI_SELECT_MAX_RANKS) * genphi::kSelectDigits);
    } catch (const std::bad_alloc &) {
        return genphi_set_error(GENPHI_ERR_ALLOC, std::string(name) + ": no host memory for the tables");
    }
    const size_t max_cells = static_cast<size_t>(GENPHI_SELECT_MAX_RANKS) * genphi::kSelectDigits;
    const genphi::HistScratch s = genphi::hist_scratch(ch.order.size(), static_cast<size_t>(ch.n_chunks()), 0, 0, max_cells);
    char *scratch;
    int rc = scratch_for(p, s.total, name, "the walk order and the digit tables", &scratch);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(scratch + s.order, ch.order.data(), ch.order.size() * sizeof(int32_t), hipMemcpyHostToDevice, v.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(scratch + s.begin, ch.begin.data(), ch.begin.size() * sizeof(int32_t), hipMemcpyHostToDevice, v.stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(v.stream);
        return genphi_set_error(GENPHI_ERR_DEVICE, std::string(name) + ": " + hipGetErrorString(e));
    }
    // every rank carries the bits found so far and its rank among the entries that share them; a pass fixes the next digit
    uint32_t prefix[GENPHI_SELECT_MAX_RANKS] = {0};
    int64_t left[GENPHI_SELECT_MAX_RANKS];
    for (int32_t r = 0; r < n_ranks; ++r) left[r] = ranks[r];
    SelectArgs a;
    a.m = v.result; a.ld = static_cast<long long>(v.ld); a.n = static_cast<int>(N); a.row_begin = static_cast<int>(v.row_begin);
    a.order = reinterpret_cast<const int *>(scratch + s.order); a.begin = reinterpret_cast<const int *>(scratch + s.begin);
    a.out = reinterpret_cast<unsigned long long *>(scratch + s.table);
    for (int pass = 0; pass < genphi::kSelectPasses; ++pass) {
        a.shift = 32 - (pass + 1) * genphi::kSelectDigitBits;
        a.n_prefix = 0;
        int slot[GENPHI_SELECT_MAX_RANKS];
        for (int32_t r = 0; r < n_ranks; ++r) {                                 // the distinct prefixes, in order of first appearance
            int q = 0;
            while (q < a.n_prefix && a.prefix[q] != prefix[r]) ++q;
            if (q == a.n_prefix) a.prefix[a.n_prefix++] = prefix[r];
            slot[r] = q;
        }
        for (int q = a.n_prefix; q < GENPHI_SELECT_MAX_RANKS; ++q) a.prefix[q] = 0;
        tab.assign(static_cast<size_t>(a.n_prefix) * genphi::kSelectDigits, 0);
        e = hipMemsetAsync(scratch + s.table, 0, tab.size() * sizeof(uint64_t), v.stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL((select_kernel<GENPHI_HIST_AGG_ROUNDS>), dim3(static_cast<unsigned>(ch.n_chunks())), dim3(kThreads), 0, v.stream, a);
            e = hipGetLastError();
        }
        rc = table_back(v, e, tab, scratch + s.table, name);
        if (rc) return rc;
        for (int32_t r = 0; r < n_ranks; ++r) {
            const uint64_t *t = tab.data() + static_cast<size_t>(slot[r]) * genphi::kSelectDigits;
            int d = 0;
            int64_t rest = left[r];
            while (d < genphi::kSelectDigits && rest >= static_cast<int64_t>(t[d])) rest -= static_cast<int64_t>(t[d++]);
            if (d == genphi::kSelectDigits)
                return genphi_set_error(GENPHI_ERR_DEVICE, std::string(name) + ": pass " + std::to_string(pass) + " counted fewer entries than the rank it narrows");
            left[r] = rest;
            prefix[r] = (prefix[r] << genphi::kSelectDigitBits) | static_cast<uint32_t>(d);
        }
    }
    for (int32_t r = 0; r < n_ranks; ++r) std::memcpy(&values[r], &prefix[r], sizeof(float));
    if (n_pairs) *n_pairs = total;                                              // (outputs are written on success only)
    return GENPHI_OK;
}

}  // extern "C"
