// occ.hip -- gen.occ and gen.rec: occurrences and coverage of ancestors (include/genphi.h, genphi_occ_* / genphi_rec_*).
//
// Reference: occ(pedigree; pro, ancestors, typeOcc), src/describe.jl:184-238, walks every ascending path of every proband
// (_occur!) and increments the flagged ancestors it meets: one step per path (287,849 on genea140, about 2^29 per proband on
// cfg4).  rec(pedigree, probandIDs, ancestorIDs), src/describe.jl:133-145, searches the descendants of each ancestor and counts
// those that are probands.
//
// Here: two linear recursions over the generation cuts of the planner, on the host schedule of ancestor_sweep.h (the one gen.gc
// runs on: rows, slots, panels):
//     occ:  N[x] = N[father] + N[mother]  (a missing parent is the zero row),  then N[x][j] += 1 where ancestors[j] == x
//     rec:  R[x] = R[father] | R[mother],                                      then R[x][j]  = 1 where ancestors[j] == x
// N[x][j] = the number of ascending paths from x to ancestors[j] (the path of length 0 included), R[x][j] = "ancestors[j] is x
// or an ancestor of x".
//
// occ rows are unsigned integers added with wrap-around.  Addition modulo 2^64 commutes with the recursion, and the reference's
// Int wraps the same way, so 64-bit rows give the reference's numbers bit for bit at any depth (read as Int64).  By induction over
// the cuts N[x][j] <= 2^c for a member of cut c (a new member adds two rows of cut c - 1; the one-hot adds 1 only where both are
// 0), so a sweep of at most 31 steps is exact in unsigned 32-bit rows as well: half the bytes.  The width is chosen at plan time
// (GENPHI_OCC_ROWS64 / the hook GENPHI_OCC_ROWS=64 force 64 bits); the result is Int64 either way.
//   IND    Emit::EveryProband: the last step writes one Int64 result row (n_pro x n_anc, row-major, ld = n_anc) per occurrence
//          of every proband; probands dragged into the last cut are copied from their slots by items of the same list
//   TOTAL  the same last list, reduced on the device: every row group adds OCC_TOTAL_ROWS rows in registers and adds the sums to
//          the n_anc totals with 64-bit atomics (integer addition: the same bits on every run).  No n_pro x n_anc buffer exists.
// rec rows are bit sets, 64 ancestor columns per 64-bit word, panel by panel (bit j - p0 of a panel that starts at column p0).
// rec is NOT occ > 0: a path count can wrap to 0.  Emit::None: the probands' rows stay in their slots, and one pass counts, per
// column, the probands whose bit is set: a lane owns one word of the rows it walks and keeps 64 counters in registers
// (rec_count_kernel).  Bits past the panel's last column are never set (the one-hot is checked against the panel) and never counted.
// The strict-descendant rule (an ancestor that is a proband does not count itself) is a subtraction on the host.
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

template <typename T>
struct alignas(16) RowVec {
    T v[16 / sizeof(T)];
};

// gc_step_kernel's shape (gc.hip) over rows of T: one item = one row; LPR lanes per row (a power of two), each lane moves 16
// bytes (V elements) per access, U accesses of each source row in flight before any is used; a wave holds 64 / LPR rows.
// BITS: an element is a word of 64 columns combined with OR; else an element is a column, added with wrap-around.
// TO_RESULT (occ only): the row goes to the Int64 result, zero-extended, 8 bytes per store (rows are not 16-byte aligned when
// n_anc is odd).
template <typename T, bool BITS, int LPR, bool TO_RESULT>
__global__ void __launch_bounds__(256)
anc_step_kernel(const int4 *__restrict__ items, const int *__restrict__ oh_cols, int n_items, T *__restrict__ slots,
                long long panel_stride, int Cp, int C, int n_anc, int panel0, long long *__restrict__ out)
{
    constexpr int V = 16 / sizeof(T);
    constexpr int RPW = 64 / LPR;
    constexpr int U = 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long item = (static_cast<long long>(blockIdx.x) * 4 + wave) * RPW + lane / LPR;
    if (item >= n_items) return;
    const int l = lane % LPR;
    const int panel = panel0 + static_cast<int>(blockIdx.y);
    const int p0 = panel * C;
    const int ncols = min(C, n_anc - p0);
    const int ne = BITS ? (ncols + 63) >> 6 : ncols;       // elements of the panel's rows
    const int lim = (ne + V - 1) & ~(V - 1);               // elements moved: rounded up to 16 bytes (<= Cp)
    const int4 it = items[item];
    const int oh_b = it.w, oh_e = items[item + 1].w;
    T *base = slots + static_cast<long long>(blockIdx.y) * panel_stride;
    const RowVec<T> *rA = it.y >= 0 ? reinterpret_cast<const RowVec<T> *>(base + static_cast<long long>(it.y) * Cp) : nullptr;
    const RowVec<T> *rB = it.z >= 0 ? reinterpret_cast<const RowVec<T> *>(base + static_cast<long long>(it.z) * Cp) : nullptr;
    RowVec<T> *dst = TO_RESULT ? nullptr : reinterpret_cast<RowVec<T> *>(base + static_cast<long long>(it.x) * Cp);
    long long *orow = TO_RESULT ? out + static_cast<long long>(it.x) * n_anc + p0 : nullptr;
    for (int c0 = V * l; c0 < lim; c0 += V * LPR * U) {
        RowVec<T> a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * V * LPR;
#pragma unroll
            for (int e = 0; e < V; ++e) { a[u].v[e] = 0; b[u].v[e] = 0; }
            if (c < lim) {
                if (rA) a[u] = rA[c / V];
                if (rB) b[u] = rB[c / V];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * V * LPR;
            if (c >= lim) break;
            RowVec<T> v;
#pragma unroll
            for (int e = 0; e < V; ++e) v.v[e] = BITS ? (a[u].v[e] | b[u].v[e]) : static_cast<T>(a[u].v[e] + b[u].v[e]);
            for (int k = oh_b; k < oh_e; ++k) {
                const int j = oh_cols[k] - p0;
                if (j < 0 || j >= ncols) continue;          // another panel's column
                const int el = BITS ? j >> 6 : j;
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (el == c + e) v.v[e] = BITS ? (v.v[e] | (static_cast<T>(1) << (j & 63))) : static_cast<T>(v.v[e] + 1);
            }
            if (TO_RESULT) {
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (c + e < ncols) orow[c + e] = static_cast<long long>(static_cast<unsigned long long>(v.v[e]));
            } else {
                dst[c / V] = v;
            }
        }
    }
}

// occ TOTAL: the items of the last list, OCC_TOTAL_ROWS consecutive items per row group (LPR lanes), summed in 64-bit registers
// column by column, then one 64-bit atomic add per column and row group.
constexpr int OCC_TOTAL_ROWS = 64;

template <typename T, int LPR>
__global__ void __launch_bounds__(256)
occ_total_kernel(const int4 *__restrict__ items, const int *__restrict__ oh_cols, int n_items, const T *__restrict__ slots,
                 long long panel_stride, int Cp, int C, int n_anc, int panel0, unsigned long long *__restrict__ totals)
{
    constexpr int V = 16 / sizeof(T);
    constexpr int RPW = 64 / LPR;
    constexpr int U = 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long first = ((static_cast<long long>(blockIdx.x) * 4 + wave) * RPW + lane / LPR) * OCC_TOTAL_ROWS;
    if (first >= n_items) return;
    const int last = static_cast<int>(min(first + OCC_TOTAL_ROWS, static_cast<long long>(n_items)));
    const int l = lane % LPR;
    const int panel = panel0 + static_cast<int>(blockIdx.y);
    const int p0 = panel * C;
    const int ncols = min(C, n_anc - p0);
    const int lim = (ncols + V - 1) & ~(V - 1);
    const T *base = slots + static_cast<long long>(blockIdx.y) * panel_stride;
    for (int c0 = V * l; c0 < lim; c0 += V * LPR * U) {
        unsigned long long acc[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int e = 0; e < V; ++e) acc[u][e] = 0;
        for (int i = static_cast<int>(first); i < last; ++i) {
            const int4 it = items[i];
            const int oh_b = it.w, oh_e = items[i + 1].w;
            const RowVec<T> *rA = it.y >= 0 ? reinterpret_cast<const RowVec<T> *>(base + static_cast<long long>(it.y) * Cp) : nullptr;
            const RowVec<T> *rB = it.z >= 0 ? reinterpret_cast<const RowVec<T> *>(base + static_cast<long long>(it.z) * Cp) : nullptr;
            RowVec<T> a[U], b[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = c0 + u * V * LPR;
#pragma unroll
                for (int e = 0; e < V; ++e) { a[u].v[e] = 0; b[u].v[e] = 0; }
                if (c < lim) {
                    if (rA) a[u] = rA[c / V];
                    if (rB) b[u] = rB[c / V];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = c0 + u * V * LPR;
#pragma unroll
                for (int e = 0; e < V; ++e) acc[u][e] += static_cast<T>(a[u].v[e] + b[u].v[e]);
                for (int k = oh_b; k < oh_e; ++k) {
                    const int j = oh_cols[k] - p0;
                    if (j < 0 || j >= ncols) continue;
#pragma unroll
                    for (int e = 0; e < V; ++e)
                        if (j == c + e) acc[u][e] += 1;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * V * LPR;
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (c + e < ncols && acc[u][e]) atomicAdd(&totals[p0 + c + e], acc[u][e]);
        }
    }
}

// Totals of a resident IND result: column sums of the n_pro x n_anc Int64 matrix (a thread per column, 256 rows per block).
__global__ void __launch_bounds__(256)
occ_colsum_kernel(const long long *__restrict__ res, long long n_pro, int n_anc, unsigned long long *__restrict__ totals)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_anc) return;
    const long long r0 = static_cast<long long>(blockIdx.y) * 256, r1 = min(r0 + 256, n_pro);
    unsigned long long s = 0;
    for (long long r = r0; r < r1; ++r) s += static_cast<unsigned long long>(res[r * n_anc + j]);
    if (s) atomicAdd(&totals[j], s);
}

// rec: per column, the number of listed rows (the probands' slots) whose bit is set.  A lane owns word blockIdx.x * 64 + lane of
// the panel's rows (a wave reads 512 contiguous bytes of a row) and keeps one counter per bit; the waves of the grid's y
// dimension share the rows.  Columns past the panel's last one (the rest of its last word) are not counted.
__global__ void __launch_bounds__(256)
rec_count_kernel(const int *__restrict__ rows, int n_rows, const unsigned long long *__restrict__ slots, long long panel_stride,
                 int Cp, int C, int n_anc, int panel0, unsigned long long *__restrict__ counts)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int panel = panel0 + static_cast<int>(blockIdx.z);
    const int p0 = panel * C;
    const int ncols = min(C, n_anc - p0);
    const int nw = (ncols + 63) >> 6;
    const int w = static_cast<int>(blockIdx.x) * 64 + lane;
    if (w >= nw) return;
    const unsigned long long *base = slots + static_cast<long long>(blockIdx.z) * panel_stride + w;
    const int stride = static_cast<int>(gridDim.y) * 4;
    unsigned cnt[64];
#pragma unroll
    for (int b = 0; b < 64; ++b) cnt[b] = 0;
#pragma unroll 4
    for (int r = static_cast<int>(blockIdx.y) * 4 + wave; r < n_rows; r += stride) {
        const unsigned long long word = base[static_cast<long long>(rows[r]) * Cp];
        const unsigned lo = static_cast<unsigned>(word), hi = static_cast<unsigned>(word >> 32);
#pragma unroll
        for (int b = 0; b < 32; ++b) {
            cnt[b] += (lo >> b) & 1u;
            cnt[32 + b] += (hi >> b) & 1u;
        }
    }
#pragma unroll
    for (int b = 0; b < 64; ++b) {
        const int j = w * 64 + b;
        if (j < ncols && cnt[b]) atomicAdd(&counts[p0 + j], static_cast<unsigned long long>(cnt[b]));
    }
}

#define ANC_LPR_SWITCH(lpr, CALL)                      \
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
// Infinity Cache between the step that writes them and the steps that read them, one panel per launch.  occ: at least 64 columns;
// rec (1 bit per column): a multiple of 128 columns (whole 16-byte accesses), at least 4,096 (512-byte rows).
constexpr double kPanelSlotBytes = 150.0 * 1048576.0;
constexpr int64_t kPanelMinCols = 64, kRecPanelMinCols = 4096;

enum { kOccInd = 0, kOccTotal = 1, kRec = 2 };

}  // namespace

struct genphi_anc_sweep {
    int kind = kOccInd;
    int64_t n_pro = 0, n_anc = 0;
    genphi::SweepSchedule sched;             // host schedule (ancestor_sweep.h)
    int32_t panel_env = 0, group_env = 0;    // GENPHI_OCC_PANEL / GENPHI_OCC_PANELS_PER_LAUNCH (0 = default rule)
    int32_t row_bits = 64;                   // occ: 64 or 32; rec: 64 (a word of 64 columns)
    // device
    int device = -1;
    hipStream_t stream = nullptr;
    long long *d_result = nullptr;           // IND: n_pro x n_anc; TOTAL: n_anc totals; rec: n_anc counts
    unsigned long long *d_colsum = nullptr;  // IND: n_anc totals, on request
    int4 *d_items = nullptr;
    int *d_oh = nullptr, *d_rows = nullptr;
    void *d_slots = nullptr;
    size_t slot_bytes = 0;
    bool computed = false;
    double sweep_ms = 0.0, alg_bytes = 0.0;
    int32_t panel_cols = 0;
    int64_t n_launches = 0;
    size_t result_bytes() const
    {
        return (kind == kOccInd ? static_cast<size_t>(n_pro) : size_t(1)) * static_cast<size_t>(n_anc) * sizeof(long long);
    }
    bool empty() const { return n_anc == 0 || n_pro == 0; }
};
struct genphi_occ : genphi_anc_sweep {};
struct genphi_rec : genphi_anc_sweep {};

namespace {

using Sweep = genphi_anc_sweep;

void release_device(Sweep *h)
{
    if (h->device < 0) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    (void)genphi::cached_free(h->d_result);
    (void)genphi::cached_free(h->d_colsum);
    (void)genphi::cached_free(h->d_items);
    (void)genphi::cached_free(h->d_oh);
    (void)genphi::cached_free(h->d_rows);
    (void)genphi::cached_free(h->d_slots);
    h->d_result = nullptr; h->d_colsum = nullptr; h->d_items = nullptr; h->d_oh = nullptr; h->d_rows = nullptr;
    h->d_slots = nullptr; h->slot_bytes = 0;
    if (h->stream) genphi::cached_stream_release(h->stream, h->device);
    h->stream = nullptr;
    (void)hipSetDevice(cur);
    h->device = -1;
    h->computed = false;
}

#define OCC_TRY(expr)                                                                                           \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

const char *kind_name(const Sweep *h) { return h->kind == kRec ? "gen.rec" : "gen.occ"; }

int create_impl(Sweep *h, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, bool rows64)
{
    if (const char *e = genphi::env_hook("GENPHI_OCC_PANEL")) h->panel_env = std::max(0, std::atoi(e));
    if (const char *e = genphi::env_hook("GENPHI_OCC_PANELS_PER_LAUNCH")) h->group_env = std::max(0, std::atoi(e));
    if (const char *e = genphi::env_hook("GENPHI_OCC_ROWS")) rows64 = rows64 || std::atoi(e) == 64;
    genphi::SweepOptions opt;
    if (h->kind == kRec) {
        opt.emit = genphi::Emit::None;
        opt.drop_unknown_pro = true;
    } else {
        opt.emit = genphi::Emit::EveryProband;
        opt.first_onehot_only = true;
    }
    std::string err;
    const int rc = genphi::plan_sweep(h->sched, n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids, opt, err);
    if (rc) return genphi_set_error(rc, err);
    h->n_pro = h->sched.n_pro; h->n_anc = n_anc;
    // N <= 2^c in cut c: 32-bit rows are exact for sweeps of at most 31 steps
    h->row_bits = (h->kind != kRec && !rows64 && h->sched.n_steps <= 31) ? 32 : 64;
    return GENPHI_OK;
}

template <typename T, bool BITS>
void launch_list(Sweep *h, int lpr, dim3 grid, const int4 *items, int n_items, bool to_res, long long stride, int Cp, int C, int panel0)
{
    T *slots = static_cast<T *>(h->d_slots);
    const int n_anc = static_cast<int>(h->n_anc);
    if (!to_res) {
        ANC_LPR_SWITCH(lpr, (anc_step_kernel<T, BITS, LPR, false><<<grid, 256, 0, h->stream>>>(items, h->d_oh, n_items, slots, stride, Cp, C,
                                                                                              n_anc, panel0, nullptr)));
        return;
    }
    if constexpr (!BITS) {
        if (h->kind == kOccInd) {
            ANC_LPR_SWITCH(lpr, (anc_step_kernel<T, false, LPR, true><<<grid, 256, 0, h->stream>>>(items, h->d_oh, n_items, slots, stride, Cp,
                                                                                                  C, n_anc, panel0, h->d_result)));
        } else {
            ANC_LPR_SWITCH(lpr, (occ_total_kernel<T, LPR><<<grid, 256, 0, h->stream>>>(items, h->d_oh, n_items, slots, stride, Cp, C, n_anc, panel0,
                                                                                      reinterpret_cast<unsigned long long *>(h->d_result))));
        }
    }
}

int lanes_per_row(int vecs)
{
    int lpr = 1;
    while (lpr < vecs && lpr < 64) lpr *= 2;
    return lpr;
}

int compute_impl(Sweep *h, int32_t device)
{
    if (device < 0) OCC_TRY(hipGetDevice(&device));
    if (h->device >= 0 && h->device != device) release_device(h);
    OCC_TRY(hipSetDevice(device));
    h->device = device;
    h->computed = false;
    if (!h->stream) OCC_TRY(genphi::cached_stream(&h->stream));
    const bool bits = h->kind == kRec;
    const int64_t n_anc = h->n_anc;
    const size_t res_bytes = h->result_bytes();
    const std::string who = kind_name(h);
    size_t free_b = 0, total_b = 0;
    OCC_TRY(hipMemGetInfo(&free_b, &total_b));
    const double usable = 0.9 * static_cast<double>(free_b + h->slot_bytes + (h->d_result ? res_bytes : 0));
    if (static_cast<double>(res_bytes) > usable)
        return genphi_set_error(GENPHI_ERR_ALLOC, who + ": the result (" + std::to_string(res_bytes >> 20) + " MiB) does not fit on device " +
                                                      std::to_string(device));
    // panels: C columns each (GENPHI_OCC_PANEL, else the default rule), G of them per launch
    const int64_t esize = bits ? 8 : h->row_bits / 8;       // bytes of a row element
    const int64_t V = 16 / esize;
    auto elems = [&](int64_t c) { return bits ? (c + 63) / 64 : c; };
    auto pitch = [&](int64_t c) { return (elems(c) + V - 1) / V * V; };
    const int64_t S = std::max<int64_t>(h->sched.peak_slots, 1);
    const double slot_room = usable - static_cast<double>(res_bytes) - 16.0 * static_cast<double>(h->sched.items.size()) -
                             4.0 * static_cast<double>(h->sched.oh_cols.size() + h->sched.pro_slots.size()) - (64 << 20);
    int64_t C;
    if (h->panel_env > 0) C = h->panel_env;
    else if (bits) C = std::max<int64_t>(kRecPanelMinCols, static_cast<int64_t>(kPanelSlotBytes * 8.0 / static_cast<double>(S)) / 128 * 128);
    else C = std::max<int64_t>(kPanelMinCols, static_cast<int64_t>(kPanelSlotBytes / static_cast<double>(esize * S)));
    C = std::min(C, std::max<int64_t>(n_anc, 1));
    auto panel_bytes = [&](int64_t c) { return static_cast<double>(esize) * static_cast<double>(S) * static_cast<double>(pitch(c)); };
    if (h->panel_env <= 0)
        while (C > 1 && panel_bytes(C) > slot_room) C = bits ? std::max<int64_t>(1, C / 2 / 64 * 64) : (C + 1) / 2;
    if (panel_bytes(C) > slot_room)
        return genphi_set_error(GENPHI_ERR_ALLOC, who + ": " + std::to_string(S) + " slots of " + std::to_string(C) +
                                                      " columns do not fit on device " + std::to_string(device) + " beside the result");
    const int64_t n_panels = (n_anc + C - 1) / C;
    int64_t G = 1;
    if (h->panel_env > 0) G = std::max<int64_t>(1, std::min<int64_t>(n_panels, static_cast<int64_t>(slot_room / panel_bytes(C))));
    if (h->group_env > 0) G = h->group_env;
    G = std::max<int64_t>(1, std::min<int64_t>({G, n_panels, 65535, static_cast<int64_t>(slot_room / panel_bytes(C))}));
    const int Cp = static_cast<int>(pitch(C));
    const long long stride = static_cast<long long>(S) * Cp;
    const size_t need_slots = static_cast<size_t>(G) * static_cast<size_t>(stride) * static_cast<size_t>(esize);
    if (need_slots > h->slot_bytes) {
        (void)genphi::cached_free(h->d_slots);
        h->d_slots = nullptr; h->slot_bytes = 0;
        OCC_TRY(genphi::cached_malloc(&h->d_slots, need_slots));
        h->slot_bytes = need_slots;
    }
    if (!h->d_result) OCC_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_result), res_bytes));
    if (!h->d_items && !h->sched.items.empty()) {
        OCC_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_items), h->sched.items.size() * sizeof(int4)));
        OCC_TRY(hipMemcpyAsync(h->d_items, h->sched.items.data(), h->sched.items.size() * sizeof(int4), hipMemcpyHostToDevice, h->stream));
        if (!h->sched.oh_cols.empty()) {
            OCC_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_oh), h->sched.oh_cols.size() * sizeof(int)));
            OCC_TRY(hipMemcpyAsync(h->d_oh, h->sched.oh_cols.data(), h->sched.oh_cols.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        }
        if (!h->sched.pro_slots.empty()) {
            OCC_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_rows), h->sched.pro_slots.size() * sizeof(int)));
            OCC_TRY(hipMemcpyAsync(h->d_rows, h->sched.pro_slots.data(), h->sched.pro_slots.size() * sizeof(int), hipMemcpyHostToDevice,
                                   h->stream));
        }
    }
    h->panel_cols = static_cast<int32_t>(C);
    hipEvent_t e0, e1;
    OCC_TRY(hipEventCreate(&e0));
    OCC_TRY(hipEventCreate(&e1));
    OCC_TRY(hipEventRecord(e0, h->stream));
    OCC_TRY(hipMemsetAsync(h->d_result, 0, res_bytes, h->stream));
    const int lpr = lanes_per_row(static_cast<int>(pitch(C) / V));
    const int rows_per_block = 4 * (64 / lpr);
    const int n_lists = static_cast<int>(h->sched.list_to_result.size());
    const int n_rows = static_cast<int>(h->sched.pro_slots.size());
    double bytes = static_cast<double>(res_bytes);
    int64_t launches = 0;
    for (int64_t g0 = 0; g0 < n_panels; g0 += G) {
        const int64_t g = std::min<int64_t>(G, n_panels - g0);
        double row_bytes = 0.0;                               // bytes of one row over the panels of this launch
        for (int64_t p = g0; p < g0 + g; ++p) row_bytes += static_cast<double>(esize * elems(std::min<int64_t>(C, n_anc - p * C)));
        for (int k = 0; k < n_lists; ++k) {
            const int64_t b = h->sched.list_begin[k], n_items = h->sched.list_begin[k + 1] - 1 - b;
            if (n_items <= 0) continue;
            const bool to_res = h->sched.list_to_result[k];
            bytes += row_bytes * (h->sched.list_srcs[k] + (to_res ? 0.0 : static_cast<double>(n_items)));
            const int64_t units = to_res && h->kind == kOccTotal ? (n_items + OCC_TOTAL_ROWS - 1) / OCC_TOTAL_ROWS : n_items;
            const dim3 grid(static_cast<unsigned>((units + rows_per_block - 1) / rows_per_block), static_cast<unsigned>(g));
            if (bits) launch_list<unsigned long long, true>(h, lpr, grid, h->d_items + b, static_cast<int>(n_items), false, stride, Cp,
                                                            static_cast<int>(C), static_cast<int>(g0));
            else if (h->row_bits == 32) launch_list<unsigned, false>(h, lpr, grid, h->d_items + b, static_cast<int>(n_items), to_res, stride, Cp,
                                                                     static_cast<int>(C), static_cast<int>(g0));
            else launch_list<unsigned long long, false>(h, lpr, grid, h->d_items + b, static_cast<int>(n_items), to_res, stride, Cp,
                                                        static_cast<int>(C), static_cast<int>(g0));
            OCC_TRY(hipGetLastError());
            ++launches;
        }
        if (bits && n_rows > 0) {
            const int nw = static_cast<int>(elems(C));
            const dim3 grid(static_cast<unsigned>((nw + 63) / 64), static_cast<unsigned>(std::min(std::max((n_rows + 511) / 512, 1), 1024)),
                            static_cast<unsigned>(g));
            rec_count_kernel<<<grid, 256, 0, h->stream>>>(h->d_rows, n_rows, static_cast<const unsigned long long *>(h->d_slots), stride, Cp,
                                                          static_cast<int>(C), static_cast<int>(n_anc), static_cast<int>(g0),
                                                          reinterpret_cast<unsigned long long *>(h->d_result));
            OCC_TRY(hipGetLastError());
            bytes += row_bytes * static_cast<double>(n_rows);
            ++launches;
        }
    }
    OCC_TRY(hipEventRecord(e1, h->stream));
    OCC_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    OCC_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    h->sweep_ms = ms;
    h->alg_bytes = bytes;
    h->n_launches = launches;
    h->computed = true;
    return GENPHI_OK;
}

int compute_entry(Sweep *h, int32_t device, const char *fn)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, std::string(fn) + ": NULL handle");
    if (h->empty()) { h->computed = true; h->sweep_ms = 0.0; h->alg_bytes = 0.0; h->n_launches = 0; return GENPHI_OK; }
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(kind_name(h)) + ": no usable GPU");
    int rc;
    try {
        rc = compute_impl(h, device);
    } catch (const std::bad_alloc &) { rc = genphi_set_error(GENPHI_ERR_ALLOC, std::string("out of host memory in ") + kind_name(h)); }
    (void)hipSetDevice(cur);
    return rc;
}

// n 8-byte values from the device (src) to the host
int copy_out(Sweep *h, void *out, const void *src, size_t bytes)
{
    int cur = 0;
    OCC_TRY(hipGetDevice(&cur));
    OCC_TRY(hipSetDevice(h->device));
    const hipError_t e = hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, h->stream);
    const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(h->stream) : e;
    (void)hipSetDevice(cur);
    if (e2 != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(kind_name(h)) + " result copy: " + hipGetErrorString(e2));
    return GENPHI_OK;
}

int check_create_args(const char *fn, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                      const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, const void *out)
{
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, std::string(fn) + ": out is NULL");
    if (n_ind < 0 || n_pro < 0 || n_anc < 0 || (n_ind && (!ind || !father || !mother)) || (n_pro && !pro_ids) || (n_anc && !anc_ids))
        return genphi_set_error(GENPHI_ERR_ARG, std::string(fn) + ": bad sizes or NULL arrays");
    if (n_ind >= INT32_MAX || n_anc >= INT32_MAX - 64 || n_pro >= INT32_MAX)
        return genphi_set_error(GENPHI_ERR_ARG, std::string(fn) + ": more than 2^31 - 65 individuals, probands or ancestors");
    return GENPHI_OK;
}

template <typename H>
int create_entry(const char *fn, int kind, bool rows64, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                 int64_t n_pro, const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, H **out)
{
    if (out) *out = nullptr;
    if (int rc = check_create_args(fn, n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids, out)) return rc;
    H *h = new (std::nothrow) H();
    if (!h) return genphi_set_error(GENPHI_ERR_ALLOC, "out of memory");
    h->kind = kind;
    int rc;
    try {
        rc = create_impl(h, n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids, rows64);
    } catch (const std::bad_alloc &) { rc = genphi_set_error(GENPHI_ERR_ALLOC, std::string("out of memory while planning ") + kind_name(h)); }
    if (rc) { delete h; return rc; }
    *out = h;
    return GENPHI_OK;
}

int stats_impl(const Sweep *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *panel_cols, int32_t *row_bits,
               int64_t *launches)
{
    if (sweep_ms) *sweep_ms = h->sweep_ms;
    if (algorithmic_bytes) *algorithmic_bytes = h->alg_bytes;
    if (peak_slots) *peak_slots = h->sched.peak_slots;
    if (panel_cols) *panel_cols = h->panel_cols;
    if (row_bits) *row_bits = h->row_bits;
    if (launches) *launches = h->n_launches;
    return GENPHI_OK;
}

}  // namespace

extern "C" {

int genphi_occ_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                      const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, int32_t flags, genphi_occ **out)
{
    if (flags & ~(GENPHI_OCC_TOTAL_ONLY | GENPHI_OCC_ROWS64)) {
        if (out) *out = nullptr;
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_occ_create: unknown flag");
    }
    return create_entry("genphi_occ_create", (flags & GENPHI_OCC_TOTAL_ONLY) ? kOccTotal : kOccInd, (flags & GENPHI_OCC_ROWS64) != 0, n_ind, ind,
                        father, mother, n_pro, pro_ids, n_anc, anc_ids, out);
}

int genphi_occ_compute(genphi_occ *h, int32_t device) { return compute_entry(h, device, "genphi_occ_compute"); }

int genphi_occ_result_device(const genphi_occ *h, const int64_t **d_ptr, int64_t *ld)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_occ_result_device: nothing computed");
    if (h->kind != kOccInd) return genphi_set_error(GENPHI_ERR_ARG, "genphi_occ_result_device: a TOTAL-only handle has no n_pro x n_anc result");
    if (d_ptr) *d_ptr = reinterpret_cast<const int64_t *>(h->d_result);
    if (ld) *ld = h->n_anc;
    return GENPHI_OK;
}

int genphi_occ_result_to_host(genphi_occ *h, int64_t *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_occ_result_to_host: nothing computed");
    if (h->kind != kOccInd) return genphi_set_error(GENPHI_ERR_ARG, "genphi_occ_result_to_host: a TOTAL-only handle has no n_pro x n_anc result");
    if (h->empty()) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_occ_result_to_host: out is NULL");
    return copy_out(h, out, h->d_result, h->result_bytes());
}

int genphi_occ_totals(genphi_occ *h, int64_t *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_occ_totals: nothing computed");
    if (h->n_anc == 0) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_occ_totals: out is NULL");
    const size_t bytes = static_cast<size_t>(h->n_anc) * sizeof(int64_t);
    if (h->n_pro == 0) { std::memset(out, 0, bytes); return GENPHI_OK; }
    if (h->kind == kOccTotal) return copy_out(h, out, h->d_result, bytes);
    // an IND handle: column sums of the resident result
    int cur = 0;
    OCC_TRY(hipGetDevice(&cur));
    OCC_TRY(hipSetDevice(h->device));
    hipError_t e = hipSuccess;
    if (!h->d_colsum) e = genphi::cached_malloc(reinterpret_cast<void **>(&h->d_colsum), bytes);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_colsum, 0, bytes, h->stream);
    if (e == hipSuccess) {
        const dim3 grid(static_cast<unsigned>((h->n_anc + 255) / 256), static_cast<unsigned>((h->n_pro + 255) / 256));
        occ_colsum_kernel<<<grid, 256, 0, h->stream>>>(h->d_result, h->n_pro, static_cast<int>(h->n_anc), h->d_colsum);
        e = hipGetLastError();
    }
    (void)hipSetDevice(cur);
    if (e != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string("gen.occ totals: ") + hipGetErrorString(e));
    return copy_out(h, out, h->d_colsum, bytes);
}

int genphi_occ_stats(const genphi_occ *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *panel_cols,
                     int32_t *row_bits, int64_t *launches)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_occ_stats: NULL handle");
    return stats_impl(h, sweep_ms, algorithmic_bytes, peak_slots, panel_cols, row_bits, launches);
}

void genphi_occ_destroy(genphi_occ *h)
{
    if (!h) return;
    release_device(h);
    delete h;
}

int genphi_rec_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                      const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, genphi_rec **out)
{
    return create_entry("genphi_rec_create", kRec, true, n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids, out);
}

int genphi_rec_compute(genphi_rec *h, int32_t device) { return compute_entry(h, device, "genphi_rec_compute"); }

int genphi_rec_result(genphi_rec *h, int64_t *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_rec_result: nothing computed");
    if (h->n_anc == 0) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_rec_result: out is NULL");
    if (h->n_pro == 0) { std::memset(out, 0, static_cast<size_t>(h->n_anc) * sizeof(int64_t)); return GENPHI_OK; }
    if (int rc = copy_out(h, out, h->d_result, h->result_bytes())) return rc;
    // descendants are strict: an ancestor that is a proband carries its own one-hot bit
    for (int64_t j = 0; j < h->n_anc; ++j) out[j] -= h->sched.anc_is_pro[j];
    return GENPHI_OK;
}

int genphi_rec_stats(const genphi_rec *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *panel_cols,
                     int32_t *row_bits, int64_t *launches)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_rec_stats: NULL handle");
    return stats_impl(h, sweep_ms, algorithmic_bytes, peak_slots, panel_cols, row_bits, launches);
}

void genphi_rec_destroy(genphi_rec *h)
{
    if (!h) return;
    release_device(h);
    delete h;
}

}  // extern "C"
