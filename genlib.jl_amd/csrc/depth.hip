// depth.hip -- gen.depths: the number, the shortest, the longest and the mean length of the ascents (include/genphi.h, genphi_depth_*).
//
// Reference: _findDistance(pedigree, descendantID, ancestorID), src/describe.jl:241-279, returns the length of EVERY ascending path
// between a descendant and an ancestor: it enumerates every path of the descendant as a vector of IDs (_get_paths), exponential in
// the depth with an allocation per path.  gen.meioses delivers the minimum of that list and gen.occ its length; the maximum, the mean
// and an exact count are GENLIB's gen.max / gen.mean / gen.min family.
//
// Here: one more column-independent recursion on the host schedule of ancestor_sweep.h (generation cuts, slot rows, column panels), in
// exact integer arithmetic on the 16-byte elements of depth_word.h (definition, encoding and the bound of 47 steps are stated there):
//     P[x] = P[f] + P[m],  S[x] = S[f] + S[m] + P[x],  min[x] = min(min[f], min[m]) + 1,  max[x] = max(max[f], max[m]) + 1
// then P = 1, S = 0, min = max = 0 where ancestors[j] == x.  A pedigree has no cycles, so x is never its own ancestor and the one-hot
// never competes with a route: it is a plain store, as in dist.hip.  Emit::EveryProband with marked copies, as gen.meioses: a proband
// that was dragged into the last cut waits in its slot with its final row, and its copy items (source B = -2) add no step.
//
//   PAIR      the last list writes four arrays of n_pro rows (pitch ld = n_anc rounded up to 8 entries): paths Int64, mean Float64
//             (double(S) / double(P), one rounding of exact operands), min and max Int16.  Probands whose row is "none" are not in
//             the last list: the arrays are pre-filled with 0, NaN, -1, -1.
//   ANCESTOR  the last list reduced over the probands: every row group folds kDepthGroupRows consecutive items in registers and adds
//             the sums to per-ancestor accumulators (64-bit integer atomic add for P and S, 32-bit atomic max for the closeness and
//             for max + 1).  No n_pro x n_anc buffer exists.
//   PROBAND   the last list reduced over the ancestors: the LPR lanes of a row fold its columns, combine across lanes, and one lane per
//             row and panel adds into per-row accumulators with the same atomics (the panels of a launch run in different workgroups).
// Both reductions combine integers only (sums that create has bounded below 2^63, maxima of bytes), so a call gives the same bytes
// whatever the panel width, the launch geometry or the order of arrival; a finishing kernel turns the accumulators into the four
// vectors.  There are no floating-point atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <limits>

#include "sweep_device.h"
#include "depth_word.h"

namespace {

using genphi::DepthWord;

static_assert(sizeof(genphi::SweepItem) == sizeof(int4), "items are uploaded as they are and read as int4");
static_assert(sizeof(DepthWord) == 16 && alignof(DepthWord) == 16, "a lane moves one element per access");

// the four result arrays (PAIR: n_pro rows of ld entries; the reductions: vectors)
struct DepthOut {
    long long *paths;
    double *mean;
    short *min, *max;
    long long ld;
};

// the accumulators of a reduction, one entry per ancestor (ANCESTOR) or per result row (PROBAND)
struct DepthAcc {
    unsigned long long *paths, *sum;
    unsigned *close, *far;
};

constexpr int kDepthAccesses = 4;            // accesses of a source row a lane has in flight (U of the kernels)

// the element of an item's row at panel column c (global column p0 + c): the step, then the one-hot
__device__ __forceinline__ DepthWord depth_element(const DepthWord &a, const DepthWord &b, unsigned step, const int *__restrict__ oh_cols, int oh_b,
                                                   int oh_e, int p0, int c)
{
    DepthWord v = genphi::depth_step(a, b, step);
    for (int k = oh_b; k < oh_e; ++k)
        if (oh_cols[k] - p0 == c) v = genphi::depth_onehot();
    return v;
}

// anc_step_kernel's shape (occ.hip, dist.hip) on 16-byte elements: one item = one row; LPR lanes per row (a power of two), one
// element (one column) per lane and access, U accesses of each source row in flight before any is used; a wave holds 64 / LPR rows and
// consecutive lanes move consecutive 16 bytes.  The unpack is a few VALU instructions per element; the kernel is bound by memory.
// TO_RESULT: the row goes to the four result arrays, one entry per lane and array.
template <int LPR, bool TO_RESULT>
__global__ void __launch_bounds__(256)
depth_step_kernel(const int4 *__restrict__ items, const int *__restrict__ oh_cols, int n_items, DepthWord *__restrict__ slots,
                  long long panel_stride, int Cp, int C, int n_anc, int panel0, DepthOut out)
{
    constexpr int RPW = 64 / LPR;
    constexpr int U = kDepthAccesses;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long item = (static_cast<long long>(blockIdx.x) * 4 + wave) * RPW + lane / LPR;
    if (item >= n_items) return;
    const int l = lane % LPR;
    const int panel = panel0 + static_cast<int>(blockIdx.y);
    const int p0 = panel * C;
    const int ncols = min(C, n_anc - p0);                   // elements of the panel's rows (<= Cp)
    const int4 it = items[item];
    const int oh_b = it.w, oh_e = items[item + 1].w;
    DepthWord *base = slots + static_cast<long long>(blockIdx.y) * panel_stride;
    const DepthWord *rA = it.y >= 0 ? base + static_cast<long long>(it.y) * Cp : nullptr;
    const DepthWord *rB = it.z >= 0 ? base + static_cast<long long>(it.z) * Cp : nullptr;
    const unsigned step = it.z == -2 ? 0u : 1u;             // a copy item: the row is final, no meiosis is added
    DepthWord *dst = TO_RESULT ? nullptr : base + static_cast<long long>(it.x) * Cp;
    const long long o0 = TO_RESULT ? static_cast<long long>(it.x) * out.ld + p0 : 0;
    for (int c0 = l; c0 < ncols; c0 += LPR * U) {
        DepthWord a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * LPR;
            a[u] = DepthWord{0, 0}; b[u] = DepthWord{0, 0};
            if (c < ncols) {
                if (rA) a[u] = rA[c];
                if (rB) b[u] = rB[c];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * LPR;
            if (c >= ncols) break;
            const DepthWord v = depth_element(a[u], b[u], step, oh_cols, oh_b, oh_e, p0, c);
            if (TO_RESULT) {
                const unsigned long long paths = genphi::depth_paths(v);
                out.paths[o0 + c] = static_cast<long long>(paths);
                out.mean[o0 + c] = genphi::depth_mean_of(paths, v.s);
                out.min[o0 + c] = genphi::depth_min_of(genphi::depth_close(v));
                out.max[o0 + c] = genphi::depth_max_of(genphi::depth_far(v));
            } else {
                dst[c] = v;
            }
        }
    }
}

// ANCESTOR: the items of the last list, kDepthGroupRows consecutive items per row group (LPR lanes), folded in registers column by
// column (occ_total_kernel's shape), then per column and row group one atomic per field.  A row group walks its items one after the
// other, so the parallelism comes from the number of row groups: 16 items per group (occ's 64 left a last list of 10,000 items with
// 157 waves and the walk bound by latency: 325 us per launch against 36 us for the by = proband kernel on the same rows), and the
// chunks of LPR * kDepthAccesses columns of a panel are dealt to the grid's z dimension instead of being walked in turn.
constexpr int kDepthGroupRows = 16;
constexpr int kDepthMaxChunkBlocks = 16;     // the grid's z dimension at most; in a wider panel a block walks several chunks

template <int LPR>
__global__ void __launch_bounds__(256)
depth_by_ancestor_kernel(const int4 *__restrict__ items, const int *__restrict__ oh_cols, int n_items, const DepthWord *__restrict__ slots,
                         long long panel_stride, int Cp, int C, int n_anc, int panel0, DepthAcc acc)
{
    constexpr int RPW = 64 / LPR;
    constexpr int U = kDepthAccesses;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long first = ((static_cast<long long>(blockIdx.x) * 4 + wave) * RPW + lane / LPR) * kDepthGroupRows;
    if (first >= n_items) return;
    const int last = static_cast<int>(min(first + kDepthGroupRows, static_cast<long long>(n_items)));
    const int l = lane % LPR;
    const int panel = panel0 + static_cast<int>(blockIdx.y);
    const int p0 = panel * C;
    const int ncols = min(C, n_anc - p0);
    const DepthWord *base = slots + static_cast<long long>(blockIdx.y) * panel_stride;
    for (int c0 = static_cast<int>(blockIdx.z) * LPR * U + l; c0 < ncols; c0 += static_cast<int>(gridDim.z) * LPR * U) {
        unsigned long long np[U], ns[U];
        unsigned nc[U], nf[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { np[u] = 0; ns[u] = 0; nc[u] = 0; nf[u] = 0; }
        for (int i = static_cast<int>(first); i < last; ++i) {
            const int4 it = items[i];
            const int oh_b = it.w, oh_e = items[i + 1].w;
            const DepthWord *rA = it.y >= 0 ? base + static_cast<long long>(it.y) * Cp : nullptr;
            const DepthWord *rB = it.z >= 0 ? base + static_cast<long long>(it.z) * Cp : nullptr;
            const unsigned step = it.z == -2 ? 0u : 1u;
            DepthWord a[U], b[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = c0 + u * LPR;
                a[u] = DepthWord{0, 0}; b[u] = DepthWord{0, 0};
                if (c < ncols) {
                    if (rA) a[u] = rA[c];
                    if (rB) b[u] = rB[c];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = c0 + u * LPR;                 // (past ncols: the zero element, which adds nothing)
                const DepthWord v = c < ncols ? depth_element(a[u], b[u], step, oh_cols, oh_b, oh_e, p0, c) : DepthWord{0, 0};
                np[u] += genphi::depth_paths(v);
                ns[u] += static_cast<unsigned long long>(v.s);
                nc[u] = max(nc[u], genphi::depth_close(v));
                nf[u] = max(nf[u], genphi::depth_far(v));
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * LPR;
            if (c >= ncols || !np[u]) continue;             // no path: the zero element everywhere
            atomicAdd(&acc.paths[p0 + c], np[u]);
            if (ns[u]) atomicAdd(&acc.sum[p0 + c], ns[u]);
            atomicMax(&acc.close[p0 + c], nc[u]);
            atomicMax(&acc.far[p0 + c], nf[u]);
        }
    }
}

// PROBAND: depth_step_kernel's shape on the last list; a lane folds the columns it visits, the LPR lanes of a row combine (the lanes
// of a row are all active or all gone: they share the item), and lane 0 of the row adds the panel's part to the row's accumulators.
template <int LPR>
__global__ void __launch_bounds__(256)
depth_by_proband_kernel(const int4 *__restrict__ items, const int *__restrict__ oh_cols, int n_items, const DepthWord *__restrict__ slots,
                        long long panel_stride, int Cp, int C, int n_anc, int panel0, DepthAcc acc)
{
    constexpr int RPW = 64 / LPR;
    constexpr int U = kDepthAccesses;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long item = (static_cast<long long>(blockIdx.x) * 4 + wave) * RPW + lane / LPR;
    if (item >= n_items) return;
    const int l = lane % LPR;
    const int panel = panel0 + static_cast<int>(blockIdx.y);
    const int p0 = panel * C;
    const int ncols = min(C, n_anc - p0);
    const int4 it = items[item];
    const int oh_b = it.w, oh_e = items[item + 1].w;
    const DepthWord *base = slots + static_cast<long long>(blockIdx.y) * panel_stride;
    const DepthWord *rA = it.y >= 0 ? base + static_cast<long long>(it.y) * Cp : nullptr;
    const DepthWord *rB = it.z >= 0 ? base + static_cast<long long>(it.z) * Cp : nullptr;
    const unsigned step = it.z == -2 ? 0u : 1u;
    unsigned long long np = 0, ns = 0;
    unsigned nc = 0, nf = 0;
    for (int c0 = l; c0 < ncols; c0 += LPR * U) {
        DepthWord a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * LPR;
            a[u] = DepthWord{0, 0}; b[u] = DepthWord{0, 0};
            if (c < ncols) {
                if (rA) a[u] = rA[c];
                if (rB) b[u] = rB[c];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * LPR;
            if (c >= ncols) break;
            const DepthWord v = depth_element(a[u], b[u], step, oh_cols, oh_b, oh_e, p0, c);
            np += genphi::depth_paths(v);
            ns += static_cast<unsigned long long>(v.s);
            nc = max(nc, genphi::depth_close(v));
            nf = max(nf, genphi::depth_far(v));
        }
    }
#pragma unroll
    for (int off = LPR / 2; off >= 1; off >>= 1) {
        np += __shfl_xor(np, off, 64);
        ns += __shfl_xor(ns, off, 64);
        nc = max(nc, __shfl_xor(nc, off, 64));
        nf = max(nf, __shfl_xor(nf, off, 64));
    }
    if (l != 0 || !np) return;
    atomicAdd(&acc.paths[it.x], np);
    if (ns) atomicAdd(&acc.sum[it.x], ns);
    atomicMax(&acc.close[it.x], nc);
    atomicMax(&acc.far[it.x], nf);
}

// the accumulators of a reduction as the four vectors (an entry nobody added to: 0, NaN, -1, -1)
__global__ void __launch_bounds__(256)
depth_finish_kernel(long long n, DepthAcc acc, DepthOut out)
{
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long paths = acc.paths[i];
    out.paths[i] = static_cast<long long>(paths);
    out.mean[i] = genphi::depth_mean_of(paths, static_cast<long long>(acc.sum[i]));
    out.min[i] = genphi::depth_min_of(acc.close[i]);
    out.max[i] = genphi::depth_max_of(acc.far[i]);
}

// 16-byte elements, one column each; default panels (sweep_panels.h) by gc's 150 MiB rule, at least 64 columns and a multiple of 8
constexpr genphi::PanelRule kDepthPanels = {16, 1, 1, 64, 8, 8, 8};
constexpr int64_t kResultPad = 8;            // PAIR: rows of ld = n_anc rounded up to 8 entries (Int16 rows start on 16 bytes)

}  // namespace

struct genphi_depth : SweepDevice {
    int32_t by = GENPHI_DEPTH_BY_PAIR;
    int64_t n_pro = 0, n_anc = 0, ld = 0;
    genphi::SweepSchedule sched;             // host schedule (ancestor_sweep.h)
    int32_t panel_arg = 0, group_arg = 0;    // create's panel_cols / panels_per_launch (0 = default rule)
    DevBuf<char> d_result;                   // the four arrays, one after the other: paths, mean, min, max
    DevBuf<char> d_acc;                      // the reductions' accumulators: paths, sum, close, far
    DevBuf<int4> d_items;
    DevBuf<int> d_oh;
    int32_t panel_cols = 0;
    genphi_depth() { own(d_result, d_acc, d_items, d_oh); }
    int64_t rows() const { return by == GENPHI_DEPTH_BY_ANCESTOR ? 1 : n_pro; }
    int64_t cols() const { return by == GENPHI_DEPTH_BY_PROBAND ? 1 : n_anc; }
    size_t entries() const { return static_cast<size_t>(rows()) * static_cast<size_t>(ld); }                 // with the rows' padding
    size_t result_bytes() const { return entries() * 20; }
    size_t acc_entries() const { return by == GENPHI_DEPTH_BY_PAIR ? 0 : static_cast<size_t>(rows() * cols()); }
    size_t acc_bytes() const { return acc_entries() * 24; }
    DepthOut out() const
    {
        const size_t n = entries();
        char *r = d_result.get();
        return DepthOut{reinterpret_cast<long long *>(r), reinterpret_cast<double *>(r + 8 * n), reinterpret_cast<short *>(r + 16 * n),
                        reinterpret_cast<short *>(r + 18 * n), static_cast<long long>(ld)};
    }
    DepthAcc acc() const
    {
        const size_t n = acc_entries();
        char *a = d_acc.get();
        return DepthAcc{reinterpret_cast<unsigned long long *>(a), reinterpret_cast<unsigned long long *>(a + 8 * n),
                        reinterpret_cast<unsigned *>(a + 16 * n), reinterpret_cast<unsigned *>(a + 20 * n)};
    }
    bool empty() const { return n_anc == 0 || n_pro == 0; }
};

namespace {

void launch_list(genphi_depth *h, int lpr, const ListLaunch &l, const genphi::PanelLayout &L)
{
    DepthWord *slots = h->slots<DepthWord>();
    const int n_anc = static_cast<int>(h->n_anc), C = static_cast<int>(L.C);
    if (!l.to_result) {
        GENPHI_LPR_SWITCH(lpr, (depth_step_kernel<LPR, false><<<l.grid, 256, 0, h->stream>>>(l.items, h->d_oh, l.n_items, slots, L.stride, L.Cp, C, n_anc,
                                                                                            l.panel0, DepthOut{})));
    } else if (h->by == GENPHI_DEPTH_BY_PAIR) {
        GENPHI_LPR_SWITCH(lpr, (depth_step_kernel<LPR, true><<<l.grid, 256, 0, h->stream>>>(l.items, h->d_oh, l.n_items, slots, L.stride, L.Cp, C, n_anc,
                                                                                           l.panel0, h->out())));
    } else if (h->by == GENPHI_DEPTH_BY_ANCESTOR) {
        dim3 grid = l.grid;                   // z: the panel's chunks of lpr * kDepthAccesses columns
        grid.z = static_cast<unsigned>(std::min<int64_t>((L.C + lpr * kDepthAccesses - 1) / (lpr * kDepthAccesses), kDepthMaxChunkBlocks));
        GENPHI_LPR_SWITCH(lpr, (depth_by_ancestor_kernel<LPR><<<grid, 256, 0, h->stream>>>(l.items, h->d_oh, l.n_items, slots, L.stride, L.Cp, C, n_anc,
                                                                                            l.panel0, h->acc())));
    } else {
        GENPHI_LPR_SWITCH(lpr, (depth_by_proband_kernel<LPR><<<l.grid, 256, 0, h->stream>>>(l.items, h->d_oh, l.n_items, slots, L.stride, L.Cp, C, n_anc,
                                                                                           l.panel0, h->acc())));
    }
}

int compute_impl(genphi_depth *h, int32_t device)
{
    if (int rc = h->select(device)) return rc;
    const size_t res_bytes = h->result_bytes(), acc_bytes = h->acc_bytes();
    genphi::PanelLayout L;
    if (int rc = h->size_panels(L, kDepthPanels, h->sched, h->n_anc, h->panel_arg, h->group_arg, res_bytes + acc_bytes, h->d_result.get() != nullptr, "gen.depths"))
        return rc;
    GENPHI_HIP_TRY(h->d_result.reserve(res_bytes));
    if (acc_bytes) GENPHI_HIP_TRY(h->d_acc.reserve(acc_bytes));
    if (int rc = h->upload(h->d_items, h->sched.items)) return rc;
    if (int rc = h->upload(h->d_oh, h->sched.oh_cols)) return rc;
    h->panel_cols = static_cast<int32_t>(L.C);
    SweepRun run;
    if (int rc = run.begin(*h, 20.0 * static_cast<double>(h->rows()) * static_cast<double>(h->cols()))) return rc;
    const bool pair = h->by == GENPHI_DEPTH_BY_PAIR;
    if (pair) {
        // 0, NaN (all bits set), -1, -1 everywhere: the probands whose row is "none" are not in the last list
        const size_t n = h->entries();
        GENPHI_HIP_TRY(hipMemsetAsync(h->d_result, 0, 8 * n, h->stream));
        GENPHI_HIP_TRY(hipMemsetAsync(h->d_result + 8 * n, 0xFF, 12 * n, h->stream));
    } else {
        GENPHI_HIP_TRY(hipMemsetAsync(h->d_acc, 0, h->d_acc.bytes(), h->stream));
    }
    const int lpr = lanes_per_row(L.Cp);
    if (int rc = sweep_lists(run, h->sched, h->d_items, kDepthPanels, L, h->n_anc, 4 * (64 / lpr), h->by == GENPHI_DEPTH_BY_ANCESTOR ? kDepthGroupRows : 1,
                             [&](const ListLaunch &l) { launch_list(h, lpr, l, L); }))
        return rc;
    if (!pair) {
        const long long n = static_cast<long long>(h->acc_entries());
        depth_finish_kernel<<<static_cast<unsigned>((n + 255) / 256), 256, 0, h->stream>>>(n, h->acc(), h->out());
        GENPHI_HIP_TRY(hipGetLastError());
        run.bytes += 24.0 * static_cast<double>(n);
        ++run.launches;
    }
    return run.end(*h);
}

// by = proband adds over the columns: every path must have one end point
bool has_duplicates(int64_t n, const int64_t *ids)
{
    std::vector<int64_t> v(ids, ids + n);
    std::sort(v.begin(), v.end());
    return std::adjacent_find(v.begin(), v.end()) != v.end();
}

}  // namespace

extern "C" {

int genphi_depth_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro, const int64_t *pro_ids,
                        int64_t n_anc, const int64_t *anc_ids, int32_t by, int32_t panel_cols, int32_t panels_per_launch, genphi_depth **out)
{
    if (out) *out = nullptr;
    if (int rc = check_create_args("genphi_depth_create", n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids, out, INT32_MAX - 64)) return rc;
    if (by != GENPHI_DEPTH_BY_PAIR && by != GENPHI_DEPTH_BY_PROBAND && by != GENPHI_DEPTH_BY_ANCESTOR)
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_depth_create: by is none of GENPHI_DEPTH_BY_PAIR, _BY_PROBAND, _BY_ANCESTOR");
    if (panel_cols < 0 || panels_per_launch < 0)
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_depth_create: panel_cols and panels_per_launch are 0 (the default rule) or positive");
    return create_entry(out, "gen.depths", [&](genphi_depth *h) {
        h->by = by;
        h->panel_arg = panel_cols;
        h->group_arg = panels_per_launch;
        genphi::SweepOptions opt;
        opt.emit = genphi::Emit::EveryProband;
        opt.first_onehot_only = false;
        opt.mark_copies = true;
        std::string err;
        if (const int rc = genphi::plan_sweep(h->sched, n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids, opt, err)) return genphi_set_error(rc, err);
        const int64_t steps = h->sched.n_steps;
        if (steps > GENPHI_DEPTH_MAX_STEPS)
            return genphi_set_error(GENPHI_ERR_ARG, "gen.depths: a sweep of " + std::to_string(steps) + " steps; the packed path counts hold at most " +
                                                        std::to_string(GENPHI_DEPTH_MAX_STEPS) + " steps (2^47 paths per pair)");
        h->n_pro = h->sched.n_pro; h->n_anc = n_anc;
        if (by == GENPHI_DEPTH_BY_PROBAND && has_duplicates(n_anc, anc_ids))
            return genphi_set_error(GENPHI_ERR_ARG, "gen.depths: by = proband adds over the ancestors and takes no ancestor ID twice");
        if (by == GENPHI_DEPTH_BY_ANCESTOR) {
            // the sum of S over the probands: n_pro * L * 2^L at most (S <= L * 2^L per pair), kept below 2^63
            const unsigned __int128 bound = static_cast<unsigned __int128>(h->n_pro) * static_cast<unsigned>(std::max<int64_t>(steps, 1)) << steps;
            if (bound >= (static_cast<unsigned __int128>(1) << 63))
                return genphi_set_error(GENPHI_ERR_ARG, "gen.depths: by = ancestor over " + std::to_string(h->n_pro) + " probands and " + std::to_string(steps) +
                                                            " steps: the sums of the path lengths could exceed Int64");
        }
        h->ld = by == GENPHI_DEPTH_BY_PAIR ? (n_anc + kResultPad - 1) / kResultPad * kResultPad : h->cols();
        return GENPHI_OK;
    });
}

int genphi_depth_compute(genphi_depth *h, int32_t device) { return compute_entry(h, device, "genphi_depth_compute", "gen.depths", compute_impl); }

int genphi_depth_shape(const genphi_depth *h, int64_t *rows, int64_t *cols)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_depth_shape: NULL handle");
    put(rows, h->rows());
    put(cols, h->cols());
    return GENPHI_OK;
}

int genphi_depth_result_device(const genphi_depth *h, const int16_t **d_min, const int16_t **d_max, const int64_t **d_paths, const double **d_mean,
                               int64_t *ld)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_depth_result_device: nothing computed");
    const DepthOut o = h->d_result.get() ? h->out() : DepthOut{};
    put(d_min, reinterpret_cast<const int16_t *>(o.min));
    put(d_max, reinterpret_cast<const int16_t *>(o.max));
    put(d_paths, reinterpret_cast<const int64_t *>(o.paths));
    put(d_mean, o.mean);
    put(ld, h->ld);
    return GENPHI_OK;
}

int genphi_depth_result_to_host(genphi_depth *h, int16_t *min, int16_t *max, int64_t *paths, double *mean)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_depth_result_to_host: nothing computed");
    const size_t rows = static_cast<size_t>(h->rows()), cols = static_cast<size_t>(h->cols());
    if (h->empty()) {
        // nothing was computed: a reduction over an empty list has its entries all the same (0 paths)
        for (size_t i = 0; i < rows * cols; ++i) {
            if (min) min[i] = -1;
            if (max) max[i] = -1;
            if (paths) paths[i] = 0;
            if (mean) mean[i] = std::numeric_limits<double>::quiet_NaN();
        }
        return GENPHI_OK;
    }
    const DepthOut o = h->out();
    const size_t ld = static_cast<size_t>(h->ld);
    // rows of ld entries on the device, packed on the host side of the copy
    auto copy = [&](void *dst, const void *src, size_t size) { return dst ? h->copy_out_2d(dst, src, ld * size, cols * size, rows, "gen.depths") : GENPHI_OK; };
    if (int rc = copy(min, o.min, 2)) return rc;
    if (int rc = copy(max, o.max, 2)) return rc;
    if (int rc = copy(paths, o.paths, 8)) return rc;
    return copy(mean, o.mean, 8);
}

int genphi_depth_stats(const genphi_depth *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *panel_cols, int64_t *launches)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_depth_stats: NULL handle");
    h->stats(sweep_ms, algorithmic_bytes, launches);
    put(peak_slots, h->sched.peak_slots);
    put(panel_cols, h->panel_cols);
    return GENPHI_OK;
}

void genphi_depth_destroy(genphi_depth *h) { destroy_entry(h); }

}  // extern "C"
