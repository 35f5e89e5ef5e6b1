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

#include <cstring>

#include "sweep_device.h"

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

// Default panels (sweep_panels.h).  occ: at least 64 columns; rec (1 bit per column): a multiple of 128 columns (whole 16-byte
// accesses), at least 4,096 (512-byte rows), halved to multiples of 64.
constexpr genphi::PanelRule kOcc32Panels = {4, 1, 4, 64, 1, 0, 1}, kOcc64Panels = {8, 1, 2, 64, 1, 0, 1}, kRecPanels = {8, 64, 2, 4096, 128, 64, 1};

enum { kOccInd = 0, kOccTotal = 1, kRec = 2 };

}  // namespace

struct genphi_anc_sweep : SweepDevice {
    int kind = kOccInd;
    int64_t n_pro = 0, n_anc = 0;
    genphi::SweepSchedule sched;             // host schedule (ancestor_sweep.h)
    int32_t panel_env = 0, group_env = 0;    // GENPHI_OCC_PANEL / GENPHI_OCC_PANELS_PER_LAUNCH (0 = default rule)
    int32_t row_bits = 64;                   // occ: 64 or 32; rec: 64 (a word of 64 columns)
    DevBuf<long long> d_result;              // IND: n_pro x n_anc; TOTAL: n_anc totals; rec: n_anc counts
    DevBuf<unsigned long long> d_colsum;     // IND: n_anc totals, on request
    DevBuf<int4> d_items;
    DevBuf<int> d_oh, d_rows;
    int32_t panel_cols = 0;
    genphi_anc_sweep() { own(d_result, d_colsum, d_items, d_oh, d_rows); }
    size_t result_bytes() const
    {
        return (kind == kOccInd ? static_cast<size_t>(n_pro) : size_t(1)) * static_cast<size_t>(n_anc) * sizeof(long long);
    }
    bool empty() const { return n_anc == 0 || n_pro == 0; }
    const char *who() const { return kind == kRec ? "gen.rec" : "gen.occ"; }
    const genphi::PanelRule &rule() const { return kind == kRec ? kRecPanels : row_bits == 32 ? kOcc32Panels : kOcc64Panels; }
};
struct genphi_occ : genphi_anc_sweep {};
struct genphi_rec : genphi_anc_sweep {};

namespace {

using Sweep = genphi_anc_sweep;

int create_impl(Sweep *h, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, bool rows64)
{
    h->panel_env = hook_count("GENPHI_OCC_PANEL");
    h->group_env = hook_count("GENPHI_OCC_PANELS_PER_LAUNCH");
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
void launch_list(Sweep *h, int lpr, const ListLaunch &l, const genphi::PanelLayout &L)
{
    T *slots = h->slots<T>();
    const int n_anc = static_cast<int>(h->n_anc), C = static_cast<int>(L.C);
    if (!l.to_result) {
        GENPHI_LPR_SWITCH(lpr, (anc_step_kernel<T, BITS, LPR, false><<<l.grid, 256, 0, h->stream>>>(l.items, h->d_oh, l.n_items, slots, L.stride, L.Cp,
                                                                                                   C, n_anc, l.panel0, nullptr)));
        return;
    }
    if constexpr (!BITS) {
        if (h->kind == kOccInd) {
            GENPHI_LPR_SWITCH(lpr, (anc_step_kernel<T, false, LPR, true><<<l.grid, 256, 0, h->stream>>>(l.items, h->d_oh, l.n_items, slots, L.stride,
                                                                                                       L.Cp, C, n_anc, l.panel0, h->d_result)));
        } else {
            GENPHI_LPR_SWITCH(lpr, (occ_total_kernel<T, LPR><<<l.grid, 256, 0, h->stream>>>(l.items, h->d_oh, l.n_items, slots, L.stride, L.Cp, C, n_anc,
                                                                                           l.panel0, reinterpret_cast<unsigned long long *>(h->d_result.get()))));
        }
    }
}

int compute_impl(Sweep *h, int32_t device)
{
    if (int rc = h->select(device)) return rc;
    const bool bits = h->kind == kRec;
    const genphi::PanelRule &rule = h->rule();
    const size_t res_bytes = h->result_bytes();
    genphi::PanelLayout L;
    if (int rc = h->size_panels(L, rule, h->sched, h->n_anc, h->panel_env, h->group_env, res_bytes, h->d_result.get() != nullptr, h->who())) return rc;
    GENPHI_HIP_TRY(h->d_result.reserve(res_bytes / sizeof(long long)));
    if (int rc = h->upload(h->d_items, h->sched.items)) return rc;
    if (int rc = h->upload(h->d_oh, h->sched.oh_cols)) return rc;
    if (int rc = h->upload(h->d_rows, h->sched.pro_slots)) return rc;
    h->panel_cols = static_cast<int32_t>(L.C);
    SweepRun run;
    if (int rc = run.begin(*h, static_cast<double>(res_bytes))) return rc;
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_result, 0, res_bytes, h->stream));
    const int lpr = lanes_per_row(static_cast<int>(L.Cp / rule.vec_elems));
    const int n_rows = static_cast<int>(h->sched.pro_slots.size());
    auto launch = [&](const ListLaunch &l) {
        if (bits) launch_list<unsigned long long, true>(h, lpr, l, L);
        else if (h->row_bits == 32) launch_list<unsigned, false>(h, lpr, l, L);
        else launch_list<unsigned long long, false>(h, lpr, l, L);
    };
    // rec: the probands' rows of the group's panels, counted per column before the next group takes the slots
    auto count = [&](int64_t g0, int64_t g, double row_bytes) {
        if (!bits || n_rows <= 0) return GENPHI_OK;
        const int nw = static_cast<int>(rule.elems(L.C));
        const dim3 grid(static_cast<unsigned>((nw + 63) / 64), static_cast<unsigned>(std::min(std::max((n_rows + 511) / 512, 1), 1024)),
                        static_cast<unsigned>(g));
        rec_count_kernel<<<grid, 256, 0, h->stream>>>(h->d_rows, n_rows, h->slots<const unsigned long long>(), L.stride, L.Cp,
                                                      static_cast<int>(L.C), static_cast<int>(h->n_anc), static_cast<int>(g0),
                                                      reinterpret_cast<unsigned long long *>(h->d_result.get()));
        GENPHI_HIP_TRY(hipGetLastError());
        run.bytes += row_bytes * static_cast<double>(n_rows);
        ++run.launches;
        return GENPHI_OK;
    };
    if (int rc = sweep_lists(run, h->sched, h->d_items, rule, L, h->n_anc, 4 * (64 / lpr), h->kind == kOccTotal ? OCC_TOTAL_ROWS : 1, launch, count))
        return rc;
    return run.end(*h);
}

template <typename H>
int create_entry(const char *fn, int kind, bool rows64, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                 int64_t n_pro, const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, H **out)
{
    if (out) *out = nullptr;
    if (int rc = check_create_args(fn, n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids, out, INT32_MAX - 64)) return rc;
    return create_entry(out, kind == kRec ? "gen.rec" : "gen.occ", [&](H *h) {
        h->kind = kind;
        return create_impl(h, n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids, rows64);
    });
}

int stats_impl(const Sweep *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *panel_cols, int32_t *row_bits,
               int64_t *launches)
{
    h->stats(sweep_ms, algorithmic_bytes, launches);
    put(peak_slots, h->sched.peak_slots);
    put(panel_cols, h->panel_cols);
    put(row_bits, h->row_bits);
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

int genphi_occ_compute(genphi_occ *h, int32_t device) { return compute_entry(h, device, "genphi_occ_compute", "gen.occ", compute_impl); }

int genphi_occ_result_device(const genphi_occ *h, const int64_t **d_ptr, int64_t *ld)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_occ_result_device: nothing computed");
    if (h->kind != kOccInd) return genphi_set_error(GENPHI_ERR_ARG, "genphi_occ_result_device: a TOTAL-only handle has no n_pro x n_anc result");
    put(d_ptr, reinterpret_cast<const int64_t *>(h->d_result.get()));
    put(ld, h->n_anc);
    return GENPHI_OK;
}

int genphi_occ_result_to_host(genphi_occ *h, int64_t *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_occ_result_to_host: nothing computed");
    if (h->kind != kOccInd) return genphi_set_error(GENPHI_ERR_ARG, "genphi_occ_result_to_host: a TOTAL-only handle has no n_pro x n_anc result");
    if (h->empty()) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_occ_result_to_host: out is NULL");
    return h->copy_out(out, h->d_result, h->result_bytes(), "gen.occ");
}

int genphi_occ_totals(genphi_occ *h, int64_t *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_occ_totals: nothing computed");
    if (h->n_anc == 0) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_occ_totals: out is NULL");
    const size_t bytes = static_cast<size_t>(h->n_anc) * sizeof(int64_t);
    if (h->n_pro == 0) { std::memset(out, 0, bytes); return GENPHI_OK; }
    if (h->kind == kOccTotal) return h->copy_out(out, h->d_result, bytes, "gen.occ");
    // an IND handle: column sums of the resident result
    const int rc = h->on_device("gen.occ totals", [&] {
        hipError_t e = h->d_colsum.reserve(static_cast<size_t>(h->n_anc));
        if (e == hipSuccess) e = hipMemsetAsync(h->d_colsum, 0, bytes, h->stream);
        if (e != hipSuccess) return e;
        const dim3 grid(static_cast<unsigned>((h->n_anc + 255) / 256), static_cast<unsigned>((h->n_pro + 255) / 256));
        occ_colsum_kernel<<<grid, 256, 0, h->stream>>>(h->d_result, h->n_pro, static_cast<int>(h->n_anc), h->d_colsum);
        return hipGetLastError();
    });
    return rc ? rc : h->copy_out(out, h->d_colsum, bytes, "gen.occ");
}

int genphi_occ_stats(const genphi_occ *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *panel_cols,
                     int32_t *row_bits, int64_t *launches)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_occ_stats: NULL handle");
    return stats_impl(h, sweep_ms, algorithmic_bytes, peak_slots, panel_cols, row_bits, launches);
}

void genphi_occ_destroy(genphi_occ *h) { destroy_entry(h); }

int genphi_rec_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                      const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, genphi_rec **out)
{
    return create_entry("genphi_rec_create", kRec, true, n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids, out);
}

int genphi_rec_compute(genphi_rec *h, int32_t device) { return compute_entry(h, device, "genphi_rec_compute", "gen.rec", compute_impl); }

int genphi_rec_result(genphi_rec *h, int64_t *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_rec_result: nothing computed");
    if (h->n_anc == 0) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_rec_result: out is NULL");
    if (h->n_pro == 0) { std::memset(out, 0, static_cast<size_t>(h->n_anc) * sizeof(int64_t)); return GENPHI_OK; }
    if (int rc = h->copy_out(out, h->d_result, h->result_bytes(), "gen.rec")) return rc;
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

void genphi_rec_destroy(genphi_rec *h) { destroy_entry(h); }

}  // extern "C"
