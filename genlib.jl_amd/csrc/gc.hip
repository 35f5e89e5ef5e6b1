// gc.hip -- gen.gc: the genetic contribution of ancestors to probands (include/genphi.h, genphi_gc_*).
//
// Reference: gc(pedigree; pro, ancestors), src/compute.jl:518-595 (GENLIB's Congen).  For every ancestor it walks every
// descending path to every leaf below it (_contribute!, :531-540) and adds 0.5^length to the leaf; a proband's Float32
// accumulator is read into its row and reset after each ancestor.  One step per path: 287,849 paths on genea140, about 2^29 per
// leaf on cfg4.
//
// Here: the same numbers from a linear recursion over the generation cuts of the planner (build_plan, indices_only):
//     row[x] = 0.5 * (row[father] + row[mother])  (a missing parent is the zero row),  then row[x][j] = 1 for every column j with
//     ancestors[j] == x
// Row x, column j = sum over the paths from ancestors[j] down to x of 0.5^length.  Every path into cut c has at most c steps, so
// the values of cut c are multiples of 2^-c in [0, 1]: the Float64 rows are exact for up to 52 steps, and the result is rounded
// to Float32 once (see the contract in include/genphi.h).
//
// Host schedule (genphi_gc_create, no GPU): ancestor_sweep.h, shared with gen.occ and gen.rec, with gc's emission rule
// (Emit::LeafFirst): the last step writes its rows straight into the Float32 result (n_pro x n_anc, row-major, ld = n_anc); only
// the first occurrence of a leaf proband gets values; the result is cleared once before the sweep.  Slot rows are Float64.
// Column panels: the columns are independent; a sweep runs over panels of C ancestor columns (slot memory peak_slots x C x 8
// bytes per panel).  A launch can cover several panels through grid dimension y; by default panels are sized for the Infinity
// Cache and swept one after the other (kPanelSlotBytes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/genphi.h"
#include "ancestor_sweep.h"
#include "devcache.h"
#include "planner.h"

int genphi_set_error(int code, const std::string &msg);      // genphi_hip.hip

namespace {

static_assert(sizeof(genphi::SweepItem) == sizeof(int4), "items are uploaded as they are and read as int4");

// One item (genphi::SweepItem, read as an int4) = one row a launch computes.
//
// LPR lanes per row (a power of two): each lane moves 16 bytes (two Float64 columns) per access, U accesses of each source row
// in flight before any is used; a wave holds 64 / LPR rows (narrow panels: several rows per wave instead of idle lanes).
template <int LPR, bool TO_RESULT>
__global__ void __launch_bounds__(256)
gc_step_kernel(const int4 *__restrict__ items, const int *__restrict__ oh_cols, int n_items, double *__restrict__ slots,
               long long panel_stride, int Cp, int C, int n_anc, int panel0, float *__restrict__ out)
{
    constexpr int RPW = 64 / LPR;
    constexpr int U = 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long item = (static_cast<long long>(blockIdx.x) * 4 + wave) * RPW + lane / LPR;
    if (item >= n_items) return;
    const int l = lane % LPR;
    const int panel = panel0 + static_cast<int>(blockIdx.y);
    const int p0 = panel * C;
    const int ncols = min(C, n_anc - p0);
    const int lim = (ncols + 1) & ~1;                      // columns moved: the panel's, rounded up to a 16-byte pair
    const int4 it = items[item];
    const int oh_b = it.w, oh_e = items[item + 1].w;
    double *base = slots + static_cast<long long>(blockIdx.y) * panel_stride;
    const double2 *rA = it.y >= 0 ? reinterpret_cast<const double2 *>(base + static_cast<long long>(it.y) * Cp) : nullptr;
    const double2 *rB = it.z >= 0 ? reinterpret_cast<const double2 *>(base + static_cast<long long>(it.z) * Cp) : nullptr;
    double2 *dst = TO_RESULT ? nullptr : reinterpret_cast<double2 *>(base + static_cast<long long>(it.x) * Cp);
    float *orow = TO_RESULT ? out + static_cast<long long>(it.x) * n_anc + p0 : nullptr;
    for (int c0 = 2 * l; c0 < lim; c0 += 2 * LPR * U) {
        double2 a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * 2 * LPR;
            a[u] = make_double2(0.0, 0.0);
            b[u] = make_double2(0.0, 0.0);
            if (c < lim) {
                if (rA) a[u] = rA[c >> 1];
                if (rB) b[u] = rB[c >> 1];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * 2 * LPR;
            if (c >= lim) break;
            double2 v = make_double2(0.5 * (a[u].x + b[u].x), 0.5 * (a[u].y + b[u].y));
            for (int k = oh_b; k < oh_e; ++k) {
                const int j = oh_cols[k] - p0;
                if (j == c) v.x = 1.0;
                if (j == c + 1 && c + 1 < ncols) v.y = 1.0;
            }
            if (TO_RESULT) {
                // rows of the result are not 16-byte (or 8-byte) aligned when n_anc is odd: two 4-byte stores
                orow[c] = static_cast<float>(v.x);
                if (c + 1 < ncols) orow[c + 1] = static_cast<float>(v.y);
            } else {
                dst[c >> 1] = v;
            }
        }
    }
}

template <bool TO_RESULT>
void launch_step(int lpr, dim3 grid, hipStream_t st, const int4 *items, const int *oh, int n_items, double *slots, long long stride,
                 int Cp, int C, int n_anc, int panel0, float *out)
{
    switch (lpr) {
    case 1: gc_step_kernel<1, TO_RESULT><<<grid, 256, 0, st>>>(items, oh, n_items, slots, stride, Cp, C, n_anc, panel0, out); break;
    case 2: gc_step_kernel<2, TO_RESULT><<<grid, 256, 0, st>>>(items, oh, n_items, slots, stride, Cp, C, n_anc, panel0, out); break;
    case 4: gc_step_kernel<4, TO_RESULT><<<grid, 256, 0, st>>>(items, oh, n_items, slots, stride, Cp, C, n_anc, panel0, out); break;
    case 8: gc_step_kernel<8, TO_RESULT><<<grid, 256, 0, st>>>(items, oh, n_items, slots, stride, Cp, C, n_anc, panel0, out); break;
    case 16: gc_step_kernel<16, TO_RESULT><<<grid, 256, 0, st>>>(items, oh, n_items, slots, stride, Cp, C, n_anc, panel0, out); break;
    case 32: gc_step_kernel<32, TO_RESULT><<<grid, 256, 0, st>>>(items, oh, n_items, slots, stride, Cp, C, n_anc, panel0, out); break;
    default: gc_step_kernel<64, TO_RESULT><<<grid, 256, 0, st>>>(items, oh, n_items, slots, stride, Cp, C, n_anc, panel0, out); break;
    }
}

// Default panels: as wide as keeps the slot rows of one panel within about 150 MiB, so that a panel's live rows stay in the
// 256 MiB Infinity Cache between the step that writes them and the steps that read them; one panel per launch, panels one after
// the other.  Measured against one panel of every column: cfg3 x 6,633 founders 1.53 vs 1.96 ms, cfg4 x
// 50,366 founders 122 vs 140 ms.  Narrower than kPanelMinCols the rows get too short for the 16-byte row gather.
constexpr double kPanelSlotBytes = 150.0 * 1048576.0;
constexpr int64_t kPanelMinCols = 64;

}  // namespace

struct genphi_gc {
    int64_t n_pro = 0, n_anc = 0;
    genphi::SweepSchedule sched;             // host schedule (ancestor_sweep.h, Emit::LeafFirst)
    int32_t panel_env = 0, group_env = 0;    // GENPHI_GC_PANEL / GENPHI_GC_PANELS_PER_LAUNCH (0 = default rule)
    // device
    int device = -1;
    hipStream_t stream = nullptr;
    float *d_result = nullptr;
    int4 *d_items = nullptr;
    int *d_oh = nullptr;
    double *d_slots = nullptr;
    size_t slot_bytes = 0;
    bool computed = false;
    double sweep_ms = 0.0, alg_bytes = 0.0;
    int32_t panel_cols = 0;
};

namespace {

void release_device(genphi_gc *h)
{
    if (h->device < 0) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    (void)genphi::cached_free(h->d_result);
    (void)genphi::cached_free(h->d_items);
    (void)genphi::cached_free(h->d_oh);
    (void)genphi::cached_free(h->d_slots);
    h->d_result = nullptr; h->d_items = nullptr; h->d_oh = nullptr; h->d_slots = nullptr; h->slot_bytes = 0;
    if (h->stream) genphi::cached_stream_release(h->stream, h->device);
    h->stream = nullptr;
    (void)hipSetDevice(cur);
    h->device = -1;
    h->computed = false;
}

#define GC_TRY(expr)                                                                                            \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

int plan_gc(genphi_gc *h, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
            const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids)
{
    genphi::SweepOptions opt;
    opt.emit = genphi::Emit::LeafFirst;
    std::string err;
    const int rc = genphi::plan_sweep(h->sched, n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids, opt, err);
    if (rc) return genphi_set_error(rc, err);
    h->n_pro = n_pro; h->n_anc = n_anc;
    return GENPHI_OK;
}

int lanes_per_row(int C)
{
    const int pairs = (C + 1) / 2;
    int lpr = 1;
    while (lpr < pairs && lpr < 64) lpr *= 2;
    return lpr;
}

int compute_impl(genphi_gc *h, int32_t device)
{
    if (device < 0) GC_TRY(hipGetDevice(&device));
    if (h->device >= 0 && h->device != device) release_device(h);
    GC_TRY(hipSetDevice(device));
    h->device = device;
    h->computed = false;
    if (!h->stream) GC_TRY(genphi::cached_stream(&h->stream));
    const int64_t n_pro = h->n_pro, n_anc = h->n_anc;
    const size_t res_bytes = static_cast<size_t>(n_pro) * static_cast<size_t>(n_anc) * sizeof(float);
    size_t free_b = 0, total_b = 0;
    GC_TRY(hipMemGetInfo(&free_b, &total_b));
    const double usable = 0.9 * static_cast<double>(free_b + h->slot_bytes + (h->d_result ? res_bytes : 0));
    if (static_cast<double>(res_bytes) > usable)
        return genphi_set_error(GENPHI_ERR_ALLOC, "gen.gc: the result (" + std::to_string(res_bytes >> 20) + " MiB) does not fit on device " +
                                                      std::to_string(device));
    // panels: C columns each (GENPHI_GC_PANEL, else the default rule), G of them per launch (as many as the memory holds)
    const int64_t S = std::max<int64_t>(h->sched.peak_slots, 1);
    const double slot_room = usable - static_cast<double>(res_bytes) -
                             16.0 * static_cast<double>(h->sched.items.size()) - 4.0 * static_cast<double>(h->sched.oh_cols.size()) - (64 << 20);
    int64_t C = h->panel_env > 0 ? h->panel_env : std::max<int64_t>(kPanelMinCols, static_cast<int64_t>(kPanelSlotBytes / (8.0 * S)));
    C = std::min(C, std::max<int64_t>(n_anc, 1));
    auto panel_bytes = [&](int64_t c) { return 8.0 * static_cast<double>(S) * static_cast<double>((c + 1) & ~int64_t(1)); };
    if (h->panel_env <= 0)
        while (C > 1 && panel_bytes(C) > slot_room) C = (C + 1) / 2;          // (more slot rows than the device holds at that width)
    if (panel_bytes(C) > slot_room)
        return genphi_set_error(GENPHI_ERR_ALLOC, "gen.gc: " + std::to_string(S) + " slots of " + std::to_string(C) +
                                                      " columns do not fit on device " + std::to_string(device) + " beside the result");
    const int64_t n_panels = n_anc > 0 ? (n_anc + C - 1) / C : 0;
    // panels per launch: one by default (see kPanelSlotBytes); with GENPHI_GC_PANEL as many as the memory holds, unless
    // GENPHI_GC_PANELS_PER_LAUNCH says otherwise (A/B and test hooks)
    int64_t G = 1;
    if (h->panel_env > 0) G = std::max<int64_t>(1, std::min<int64_t>(n_panels, static_cast<int64_t>(slot_room / panel_bytes(C))));
    if (h->group_env > 0) G = h->group_env;
    G = std::max<int64_t>(1, std::min<int64_t>({G, n_panels, 65535, static_cast<int64_t>(slot_room / panel_bytes(C))}));
    const int Cp = static_cast<int>((C + 1) & ~int64_t(1));
    const long long stride = static_cast<long long>(S) * Cp;
    const size_t need_slots = static_cast<size_t>(G) * static_cast<size_t>(stride) * sizeof(double);
    if (need_slots > h->slot_bytes) {
        (void)genphi::cached_free(h->d_slots);
        h->d_slots = nullptr; h->slot_bytes = 0;
        GC_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_slots), need_slots));
        h->slot_bytes = need_slots;
    }
    if (!h->d_result && res_bytes) GC_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_result), res_bytes));
    if (!h->d_items && !h->sched.items.empty()) {
        GC_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_items), h->sched.items.size() * sizeof(int4)));
        GC_TRY(hipMemcpyAsync(h->d_items, h->sched.items.data(), h->sched.items.size() * sizeof(int4), hipMemcpyHostToDevice, h->stream));
        if (!h->sched.oh_cols.empty()) {
            GC_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_oh), h->sched.oh_cols.size() * sizeof(int)));
            GC_TRY(hipMemcpyAsync(h->d_oh, h->sched.oh_cols.data(), h->sched.oh_cols.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        }
    }
    h->panel_cols = static_cast<int32_t>(C);
    hipEvent_t e0, e1;
    GC_TRY(hipEventCreate(&e0));
    GC_TRY(hipEventCreate(&e1));
    GC_TRY(hipEventRecord(e0, h->stream));
    if (res_bytes) GC_TRY(hipMemsetAsync(h->d_result, 0, res_bytes, h->stream));
    const int lpr = lanes_per_row(static_cast<int>(C));
    const int rows_per_block = 4 * (64 / lpr);
    const int n_lists = static_cast<int>(h->sched.list_to_result.size());
    double bytes = static_cast<double>(res_bytes);
    for (int64_t g0 = 0; g0 < n_panels; g0 += G) {
        const int64_t g = std::min<int64_t>(G, n_panels - g0);
        double cols = 0.0;                                     // columns of the panels of this launch
        for (int64_t p = g0; p < g0 + g; ++p) cols += static_cast<double>(std::min<int64_t>(C, n_anc - p * C));
        for (int k = 0; k < n_lists; ++k) {
            const int64_t b = h->sched.list_begin[k], n_items = h->sched.list_begin[k + 1] - 1 - b;
            if (n_items <= 0) continue;
            const bool to_res = h->sched.list_to_result[k];
            bytes += cols * (8.0 * h->sched.list_srcs[k] + (to_res ? 0.0 : 8.0 * static_cast<double>(n_items)));
            const dim3 grid(static_cast<unsigned>((n_items + rows_per_block - 1) / rows_per_block), static_cast<unsigned>(g));
            if (to_res)
                launch_step<true>(lpr, grid, h->stream, h->d_items + b, h->d_oh, static_cast<int>(n_items), h->d_slots, stride, Cp,
                                  static_cast<int>(C), static_cast<int>(n_anc), static_cast<int>(g0), h->d_result);
            else
                launch_step<false>(lpr, grid, h->stream, h->d_items + b, h->d_oh, static_cast<int>(n_items), h->d_slots, stride, Cp,
                                   static_cast<int>(C), static_cast<int>(n_anc), static_cast<int>(g0), h->d_result);
            GC_TRY(hipGetLastError());
        }
    }
    GC_TRY(hipEventRecord(e1, h->stream));
    GC_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    GC_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    h->sweep_ms = ms;
    h->alg_bytes = bytes;
    h->computed = true;
    return GENPHI_OK;
}

}  // namespace

extern "C" {

int genphi_gc_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                     const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, genphi_gc **out)
{
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_create: out is NULL");
    *out = nullptr;
    if (n_ind < 0 || n_pro < 0 || n_anc < 0 || (n_ind && (!ind || !father || !mother)) || (n_pro && !pro_ids) || (n_anc && !anc_ids))
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_create: bad sizes or NULL arrays");
    if (n_ind >= INT32_MAX || n_anc >= INT32_MAX || n_pro >= INT32_MAX)
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_create: more than 2^31 - 1 individuals, probands or ancestors");
    genphi_gc *h = new (std::nothrow) genphi_gc();
    if (!h) return genphi_set_error(GENPHI_ERR_ALLOC, "out of memory");
    if (const char *e = genphi::env_hook("GENPHI_GC_PANEL")) h->panel_env = std::max(0, std::atoi(e));
    if (const char *e = genphi::env_hook("GENPHI_GC_PANELS_PER_LAUNCH")) h->group_env = std::max(0, std::atoi(e));
    int rc;
    try {
        rc = plan_gc(h, n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids);
    } catch (const std::bad_alloc &) { rc = genphi_set_error(GENPHI_ERR_ALLOC, "out of memory while planning gen.gc"); }
    if (rc) { delete h; return rc; }
    *out = h;
    return GENPHI_OK;
}

int genphi_gc_compute(genphi_gc *h, int32_t device)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_compute: NULL handle");
    if (h->n_pro == 0 || h->n_anc == 0) { h->computed = true; h->sweep_ms = 0.0; h->alg_bytes = 0.0; return GENPHI_OK; }
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, "gen.gc: no usable GPU");
    int rc;
    try {
        rc = compute_impl(h, device);
    } catch (const std::bad_alloc &) { rc = genphi_set_error(GENPHI_ERR_ALLOC, "out of host memory in gen.gc"); }
    (void)hipSetDevice(cur);
    return rc;
}

int genphi_gc_result_device(const genphi_gc *h, const float **d_ptr, int64_t *ld)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_result_device: nothing computed");
    if (d_ptr) *d_ptr = h->d_result;
    if (ld) *ld = h->n_anc;
    return GENPHI_OK;
}

int genphi_gc_result_to_host(genphi_gc *h, float *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_result_to_host: nothing computed");
    const size_t bytes = static_cast<size_t>(h->n_pro) * static_cast<size_t>(h->n_anc) * sizeof(float);
    if (!bytes) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_result_to_host: out is NULL");
    int cur = 0;
    GC_TRY(hipGetDevice(&cur));
    GC_TRY(hipSetDevice(h->device));
    const hipError_t e = hipMemcpyAsync(out, h->d_result, bytes, hipMemcpyDeviceToHost, h->stream);
    const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(h->stream) : e;
    (void)hipSetDevice(cur);
    if (e2 != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string("gen.gc result copy: ") + hipGetErrorString(e2));
    return GENPHI_OK;
}

int genphi_gc_stats(const genphi_gc *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *panel_cols)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_stats: NULL handle");
    if (sweep_ms) *sweep_ms = h->sweep_ms;
    if (algorithmic_bytes) *algorithmic_bytes = h->alg_bytes;
    if (peak_slots) *peak_slots = h->sched.peak_slots;
    if (panel_cols) *panel_cols = h->panel_cols;
    return GENPHI_OK;
}

void genphi_gc_destroy(genphi_gc *h)
{
    if (!h) return;
    release_device(h);
    delete h;
}

}  // extern "C"
