// dist.hip -- gen.meioses / gen.findMRCA: shortest ascents (include/genphi.h, genphi_dist_*).
//
// Reference: findMRCA(pedigree, IDs), src/identify.jl:97-160, asks _findMinDistance (src/describe.jl:241-289) for every
// (individual, ancestor) pair; that enumerates every ascending path of the individual as a vector of IDs (_get_paths) and keeps
// the shortest one that starts at the ancestor: gen.occ's path walk with an allocation per path.
//
// Here: the fourth recursion on the host schedule of ancestor_sweep.h (generation cuts, slot rows, column panels), min-plus:
//     D[x] = min(D[father], D[mother]) + 1   ("none" is absorbing),   then D[x][j] = 0 where ancestors[j] == x
// D[x][j] = the meioses of the shortest ascending path from x to ancestors[j].
//
// Encoding.  In the schedule the row of an unrelated member, a missing parent (source -1) and a member that is never computed are
// all the zero row, so "none" has to be 0.  Rows hold the CLOSENESS c = K - d in unsigned 16 bits, K = 65535, c = 0 for none:
//     c[x] = max(c[father], c[mother]) (-) 1   (saturating at 0: none stays none),   then c[x][j] = K where ancestors[j] == x
// A pedigree has no cycles, so x is never its own ancestor and the one-hot never competes with a route: it is a plain store.
// The result is signed 16-bit, d = K - c = ~c, which reads -1 exactly where c = 0: the conversion of the last list is one NOT
// per element.  d <= the number of steps, so create refuses sweeps of more than GENPHI_DIST_MAX_STEPS = 32767 steps (d would
// not fit the signed result).  Probands whose row is "none" are not in the last list: the result is pre-filled with -1 (0xFF).
//
// Emit::EveryProband, as gen.occ: one result row per occurrence of every proband.  A proband that was dragged into the last cut
// waits in its slot with its final row; its copy items (SweepOptions::mark_copies: source B = -2) are converted without the step.
//
// The device result has a row pitch of n_anc rounded up to 8 entries, so every row starts on 16 bytes and a lane stores the 8
// entries it computed with one access when the panel starts on a multiple of 8 columns (the default panels do); the entries of
// the padding are never read.  result_to_host packs the rows (a 2-D copy).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
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

typedef unsigned short us8 __attribute__((ext_vector_type(8)));     // 16 bytes: what a lane moves per access
constexpr unsigned short kNear = 0xFFFF;                            // K: the closeness of an individual to itself

// anc_step_kernel's shape (occ.hip) on closeness rows: one item = one row; LPR lanes per row (a power of two), 8 columns per lane
// and access, U accesses of each source row in flight before any is used; a wave holds 64 / LPR rows.  The arithmetic is
// v_pk_max_u16 and v_pk_sub_u16 with clamp: 8 VALU instructions per 16 bytes.
// TO_RESULT: the row goes to the signed 16-bit result as ~c (ld entries per row); ALIGNED: the panel starts on a multiple of 8
// columns, the lane's 8 entries are one 16-byte store (the row's padding takes what lies past n_anc).
template <int LPR, bool TO_RESULT, bool ALIGNED>
__global__ void __launch_bounds__(256)
dist_step_kernel(const int4 *__restrict__ items, const int *__restrict__ oh_cols, int n_items, unsigned short *__restrict__ slots,
                 long long panel_stride, int Cp, int C, int n_anc, int panel0, short *__restrict__ out, long long ld)
{
    constexpr int V = 8;
    constexpr int RPW = 64 / LPR;
    constexpr int U = 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long item = (static_cast<long long>(blockIdx.x) * 4 + wave) * RPW + lane / LPR;
    if (item >= n_items) return;
    const int l = lane % LPR;
    const int panel = panel0 + static_cast<int>(blockIdx.y);
    const int p0 = panel * C;
    const int ncols = min(C, n_anc - p0);
    const int lim = (ncols + V - 1) & ~(V - 1);            // columns moved: rounded up to 16 bytes (<= Cp)
    const int4 it = items[item];
    const int oh_b = it.w, oh_e = items[item + 1].w;
    unsigned short *base = slots + static_cast<long long>(blockIdx.y) * panel_stride;
    const us8 *rA = it.y >= 0 ? reinterpret_cast<const us8 *>(base + static_cast<long long>(it.y) * Cp) : nullptr;
    const us8 *rB = it.z >= 0 ? reinterpret_cast<const us8 *>(base + static_cast<long long>(it.z) * Cp) : nullptr;
    const us8 step = it.z == -2 ? us8(0) : us8(1);          // a copy item: the row is final, no meiosis is added
    us8 *dst = TO_RESULT ? nullptr : reinterpret_cast<us8 *>(base + static_cast<long long>(it.x) * Cp);
    short *orow = TO_RESULT ? out + static_cast<long long>(it.x) * ld + p0 : nullptr;
    for (int c0 = V * l; c0 < lim; c0 += V * LPR * U) {
        us8 a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * V * LPR;
            a[u] = us8(0); b[u] = us8(0);
            if (c < lim) {
                if (rA) a[u] = rA[c / V];
                if (rB) b[u] = rB[c / V];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * V * LPR;
            if (c >= lim) break;
            us8 v = __builtin_elementwise_sub_sat(__builtin_elementwise_max(a[u], b[u]), step);
            for (int k = oh_b; k < oh_e; ++k) {
                const int j = oh_cols[k] - p0;
                if (j < 0 || j >= ncols) continue;          // another panel's column
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (j == c + e) v[e] = kNear;
            }
            if (TO_RESULT) {
                const us8 d = ~v;
                if (ALIGNED) {
                    *reinterpret_cast<us8 *>(orow + c) = d;
                } else {
#pragma unroll
                    for (int e = 0; e < V; ++e)
                        if (c + e < ncols) orow[c + e] = static_cast<short>(d[e]);
                }
            } else {
                dst[c / V] = v;
            }
        }
    }
}

#define DIST_LPR_SWITCH(lpr, CALL)                     \
    switch (lpr) {                                     \
    case 1: { constexpr int LPR = 1; CALL; } break;    \
    case 2: { constexpr int LPR = 2; CALL; } break;    \
    case 4: { constexpr int LPR = 4; CALL; } break;    \
    case 8: { constexpr int LPR = 8; CALL; } break;    \
    case 16: { constexpr int LPR = 16; CALL; } break;  \
    case 32: { constexpr int LPR = 32; CALL; } break;  \
    default: { constexpr int LPR = 64; CALL; } break;  \
    }

// Default panels: gc's rule (gc.hip): the slot rows of one panel within about 150 MiB so that they stay in the
// Infinity Cache between the step that writes them and the steps that read them, one panel per launch; at least 64 columns, a
// multiple of 8 (16-byte result stores).
constexpr double kPanelSlotBytes = 150.0 * 1048576.0;
constexpr int64_t kPanelMinCols = 64;
constexpr int64_t kRowBytes = 2, kVec = 8;

}  // namespace

struct genphi_dist {
    int64_t n_pro = 0, n_anc = 0, ld = 0;
    genphi::SweepSchedule sched;             // host schedule (ancestor_sweep.h)
    int32_t panel_env = 0, group_env = 0;    // GENPHI_DIST_PANEL / GENPHI_DIST_PANELS_PER_LAUNCH (0 = default rule)
    // device
    int device = -1;
    hipStream_t stream = nullptr;
    short *d_result = nullptr;               // n_pro rows of ld entries
    int4 *d_items = nullptr;
    int *d_oh = nullptr;
    unsigned short *d_slots = nullptr;
    size_t slot_bytes = 0;
    bool computed = false;
    double sweep_ms = 0.0, alg_bytes = 0.0;
    int32_t panel_cols = 0;
    int64_t n_launches = 0;
    size_t result_bytes() const { return static_cast<size_t>(n_pro) * static_cast<size_t>(ld) * sizeof(short); }
    bool empty() const { return n_anc == 0 || n_pro == 0; }
};

namespace {

void release_device(genphi_dist *h)
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

#define DIST_TRY(expr)                                                                                          \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

void launch_list(genphi_dist *h, int lpr, dim3 grid, const int4 *items, int n_items, bool to_res, bool aligned, long long stride, int Cp,
                 int C, int panel0)
{
    const int n_anc = static_cast<int>(h->n_anc);
    if (!to_res) {
        DIST_LPR_SWITCH(lpr, (dist_step_kernel<LPR, false, false><<<grid, 256, 0, h->stream>>>(items, h->d_oh, n_items, h->d_slots, stride, Cp, C,
                                                                                             n_anc, panel0, nullptr, 0)));
    } else if (aligned) {
        DIST_LPR_SWITCH(lpr, (dist_step_kernel<LPR, true, true><<<grid, 256, 0, h->stream>>>(items, h->d_oh, n_items, h->d_slots, stride, Cp, C,
                                                                                           n_anc, panel0, h->d_result, h->ld)));
    } else {
        DIST_LPR_SWITCH(lpr, (dist_step_kernel<LPR, true, false><<<grid, 256, 0, h->stream>>>(items, h->d_oh, n_items, h->d_slots, stride, Cp, C,
                                                                                            n_anc, panel0, h->d_result, h->ld)));
    }
}

int lanes_per_row(int vecs)
{
    int lpr = 1;
    while (lpr < vecs && lpr < 64) lpr *= 2;
    return lpr;
}

int compute_impl(genphi_dist *h, int32_t device)
{
    if (device < 0) DIST_TRY(hipGetDevice(&device));
    if (h->device >= 0 && h->device != device) release_device(h);
    DIST_TRY(hipSetDevice(device));
    h->device = device;
    h->computed = false;
    if (!h->stream) DIST_TRY(genphi::cached_stream(&h->stream));
    const int64_t n_anc = h->n_anc;
    const size_t res_bytes = h->result_bytes();
    size_t free_b = 0, total_b = 0;
    DIST_TRY(hipMemGetInfo(&free_b, &total_b));
    const double usable = 0.9 * static_cast<double>(free_b + h->slot_bytes + (h->d_result ? res_bytes : 0));
    if (static_cast<double>(res_bytes) > usable)
        return genphi_set_error(GENPHI_ERR_ALLOC, "gen.meioses: the result (" + std::to_string(res_bytes >> 20) + " MiB) does not fit on device " +
                                                      std::to_string(device));
    // panels: C columns each (GENPHI_DIST_PANEL, else the default rule), G of them per launch
    auto pitch = [&](int64_t c) { return (c + kVec - 1) / kVec * kVec; };
    const int64_t S = std::max<int64_t>(h->sched.peak_slots, 1);
    const double slot_room = usable - static_cast<double>(res_bytes) - 16.0 * static_cast<double>(h->sched.items.size()) -
                             4.0 * static_cast<double>(h->sched.oh_cols.size()) - (64 << 20);
    int64_t C;
    if (h->panel_env > 0) C = h->panel_env;
    else C = std::max<int64_t>(kPanelMinCols, static_cast<int64_t>(kPanelSlotBytes / static_cast<double>(kRowBytes * S)) / kVec * kVec);
    C = std::min(C, std::max<int64_t>(n_anc, 1));
    auto panel_bytes = [&](int64_t c) { return static_cast<double>(kRowBytes) * static_cast<double>(S) * static_cast<double>(pitch(c)); };
    if (h->panel_env <= 0)
        while (C > kVec && panel_bytes(C) > slot_room) C = std::max<int64_t>(kVec, C / 2 / kVec * kVec);
    if (panel_bytes(C) > slot_room)
        return genphi_set_error(GENPHI_ERR_ALLOC, "gen.meioses: " + std::to_string(S) + " slots of " + std::to_string(C) +
                                                      " columns do not fit on device " + std::to_string(device) + " beside the result");
    const int64_t n_panels = (n_anc + C - 1) / C;
    int64_t G = 1;
    if (h->panel_env > 0) G = std::max<int64_t>(1, std::min<int64_t>(n_panels, static_cast<int64_t>(slot_room / panel_bytes(C))));
    if (h->group_env > 0) G = h->group_env;
    G = std::max<int64_t>(1, std::min<int64_t>({G, n_panels, 65535, static_cast<int64_t>(slot_room / panel_bytes(C))}));
    const int Cp = static_cast<int>(pitch(C));
    const long long stride = static_cast<long long>(S) * Cp;
    const size_t need_slots = static_cast<size_t>(G) * static_cast<size_t>(stride) * static_cast<size_t>(kRowBytes);
    if (need_slots > h->slot_bytes) {
        (void)genphi::cached_free(h->d_slots);
        h->d_slots = nullptr; h->slot_bytes = 0;
        DIST_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_slots), need_slots));
        h->slot_bytes = need_slots;
    }
    if (!h->d_result) DIST_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_result), res_bytes));
    if (!h->d_items && !h->sched.items.empty()) {
        DIST_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_items), h->sched.items.size() * sizeof(int4)));
        DIST_TRY(hipMemcpyAsync(h->d_items, h->sched.items.data(), h->sched.items.size() * sizeof(int4), hipMemcpyHostToDevice, h->stream));
        if (!h->sched.oh_cols.empty()) {
            DIST_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_oh), h->sched.oh_cols.size() * sizeof(int)));
            DIST_TRY(hipMemcpyAsync(h->d_oh, h->sched.oh_cols.data(), h->sched.oh_cols.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        }
    }
    h->panel_cols = static_cast<int32_t>(C);
    hipEvent_t e0, e1;
    DIST_TRY(hipEventCreate(&e0));
    DIST_TRY(hipEventCreate(&e1));
    DIST_TRY(hipEventRecord(e0, h->stream));
    // -1 everywhere: the probands whose row is "none" are not in the last list
    DIST_TRY(hipMemsetAsync(h->d_result, 0xFF, res_bytes, h->stream));
    const int lpr = lanes_per_row(static_cast<int>(pitch(C) / kVec));
    const int rows_per_block = 4 * (64 / lpr);
    const int n_lists = static_cast<int>(h->sched.list_to_result.size());
    const bool aligned = C % kVec == 0 || n_panels == 1;      // every panel starts on a multiple of 8 columns
    double bytes = static_cast<double>(h->n_pro) * static_cast<double>(n_anc) * sizeof(short);
    int64_t launches = 0;
    for (int64_t g0 = 0; g0 < n_panels; g0 += G) {
        const int64_t g = std::min<int64_t>(G, n_panels - g0);
        double row_bytes = 0.0;                               // bytes of one row over the panels of this launch
        for (int64_t p = g0; p < g0 + g; ++p) row_bytes += static_cast<double>(kRowBytes * std::min<int64_t>(C, n_anc - p * C));
        for (int k = 0; k < n_lists; ++k) {
            const int64_t b = h->sched.list_begin[k], n_items = h->sched.list_begin[k + 1] - 1 - b;
            if (n_items <= 0) continue;
            const bool to_res = h->sched.list_to_result[k];
            bytes += row_bytes * (h->sched.list_srcs[k] + (to_res ? 0.0 : static_cast<double>(n_items)));
            const dim3 grid(static_cast<unsigned>((n_items + rows_per_block - 1) / rows_per_block), static_cast<unsigned>(g));
            launch_list(h, lpr, grid, h->d_items + b, static_cast<int>(n_items), to_res, aligned, stride, Cp, static_cast<int>(C),
                        static_cast<int>(g0));
            DIST_TRY(hipGetLastError());
            ++launches;
        }
    }
    DIST_TRY(hipEventRecord(e1, h->stream));
    DIST_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    DIST_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    h->sweep_ms = ms;
    h->alg_bytes = bytes;
    h->n_launches = launches;
    h->computed = true;
    return GENPHI_OK;
}

}  // namespace

extern "C" {

int genphi_dist_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                       const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, genphi_dist **out)
{
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_dist_create: out is NULL");
    *out = nullptr;
    if (n_ind < 0 || n_pro < 0 || n_anc < 0 || (n_ind && (!ind || !father || !mother)) || (n_pro && !pro_ids) || (n_anc && !anc_ids))
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_dist_create: bad sizes or NULL arrays");
    if (n_ind >= INT32_MAX || n_anc >= INT32_MAX - 64 || n_pro >= INT32_MAX)
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_dist_create: more than 2^31 - 65 individuals, probands or ancestors");
    genphi_dist *h = new (std::nothrow) genphi_dist();
    if (!h) return genphi_set_error(GENPHI_ERR_ALLOC, "out of memory");
    int rc;
    try {
        if (const char *e = genphi::env_hook("GENPHI_DIST_PANEL")) h->panel_env = std::max(0, std::atoi(e));
        if (const char *e = genphi::env_hook("GENPHI_DIST_PANELS_PER_LAUNCH")) h->group_env = std::max(0, std::atoi(e));
        genphi::SweepOptions opt;
        opt.emit = genphi::Emit::EveryProband;
        opt.first_onehot_only = false;
        opt.mark_copies = true;
        std::string err;
        rc = genphi::plan_sweep(h->sched, n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids, opt, err);
        if (rc) rc = genphi_set_error(rc, err);
        else if (h->sched.n_steps > GENPHI_DIST_MAX_STEPS)
            rc = genphi_set_error(GENPHI_ERR_ARG, "gen.meioses: a sweep of " + std::to_string(h->sched.n_steps) + " steps; the signed 16-bit result holds at most " +
                                                      std::to_string(GENPHI_DIST_MAX_STEPS) + " meioses");
    } catch (const std::bad_alloc &) { rc = genphi_set_error(GENPHI_ERR_ALLOC, "out of memory while planning gen.meioses"); }
    if (rc) { delete h; return rc; }
    h->n_pro = h->sched.n_pro; h->n_anc = n_anc;
    h->ld = (n_anc + kVec - 1) / kVec * kVec;
    *out = h;
    return GENPHI_OK;
}

int genphi_dist_compute(genphi_dist *h, int32_t device)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_dist_compute: NULL handle");
    if (h->empty()) { h->computed = true; h->sweep_ms = 0.0; h->alg_bytes = 0.0; h->n_launches = 0; return GENPHI_OK; }
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, "gen.meioses: no usable GPU");
    int rc;
    try {
        rc = compute_impl(h, device);
    } catch (const std::bad_alloc &) { rc = genphi_set_error(GENPHI_ERR_ALLOC, "out of host memory in gen.meioses"); }
    (void)hipSetDevice(cur);
    return rc;
}

int genphi_dist_result_device(const genphi_dist *h, const int16_t **d_ptr, int64_t *ld)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_dist_result_device: nothing computed");
    if (d_ptr) *d_ptr = h->d_result;
    if (ld) *ld = h->ld;
    return GENPHI_OK;
}

int genphi_dist_result_to_host(genphi_dist *h, int16_t *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_dist_result_to_host: nothing computed");
    if (h->empty()) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_dist_result_to_host: out is NULL");
    int cur = 0;
    DIST_TRY(hipGetDevice(&cur));
    DIST_TRY(hipSetDevice(h->device));
    const size_t width = static_cast<size_t>(h->n_anc) * sizeof(short);
    const hipError_t e = hipMemcpy2DAsync(out, width, h->d_result, static_cast<size_t>(h->ld) * sizeof(short), width,
                                          static_cast<size_t>(h->n_pro), hipMemcpyDeviceToHost, h->stream);
    const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(h->stream) : e;
    (void)hipSetDevice(cur);
    if (e2 != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string("gen.meioses result copy: ") + hipGetErrorString(e2));
    return GENPHI_OK;
}

int genphi_dist_stats(const genphi_dist *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *panel_cols,
                      int32_t *row_bits, int64_t *launches)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_dist_stats: NULL handle");
    if (sweep_ms) *sweep_ms = h->sweep_ms;
    if (algorithmic_bytes) *algorithmic_bytes = h->alg_bytes;
    if (peak_slots) *peak_slots = h->sched.peak_slots;
    if (panel_cols) *panel_cols = h->panel_cols;
    if (row_bits) *row_bits = 16;
    if (launches) *launches = h->n_launches;
    return GENPHI_OK;
}

void genphi_dist_destroy(genphi_dist *h)
{
    if (!h) return;
    release_device(h);
    delete h;
}

}  // extern "C"
