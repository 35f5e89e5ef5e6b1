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
// Cache and swept one after the other (sweep_panels.h).  The device side of the handle: sweep_device.h.
#include <hip/hip_runtime.h>

#include "sweep_device.h"

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
    GENPHI_LPR_SWITCH(lpr, (gc_step_kernel<LPR, TO_RESULT><<<grid, 256, 0, st>>>(items, oh, n_items, slots, stride, Cp, C, n_anc, panel0, out)));
}

// Float64 rows, two columns per 16 bytes; default panels (sweep_panels.h) of at least 64 columns, halved where they do not fit
constexpr genphi::PanelRule kGcPanels = {8, 1, 2, 64, 1, 0, 1};

}  // namespace

struct genphi_gc : SweepDevice {
    int64_t n_pro = 0, n_anc = 0;
    genphi::SweepSchedule sched;             // host schedule (ancestor_sweep.h, Emit::LeafFirst)
    int32_t panel_env = 0, group_env = 0;    // GENPHI_GC_PANEL / GENPHI_GC_PANELS_PER_LAUNCH (0 = default rule)
    DevBuf<float> d_result;
    DevBuf<int4> d_items;
    DevBuf<int> d_oh;
    int32_t panel_cols = 0;
    genphi_gc() { own(d_result, d_items, d_oh); }
    size_t result_bytes() const { return static_cast<size_t>(n_pro) * static_cast<size_t>(n_anc) * sizeof(float); }
    bool empty() const { return n_pro == 0 || n_anc == 0; }
};

namespace {

int compute_impl(genphi_gc *h, int32_t device)
{
    if (int rc = h->select(device)) return rc;
    const size_t res_bytes = h->result_bytes();
    genphi::PanelLayout L;
    if (int rc = h->size_panels(L, kGcPanels, h->sched, h->n_anc, h->panel_env, h->group_env, res_bytes, h->d_result.get() != nullptr, "gen.gc")) return rc;
    GENPHI_HIP_TRY(h->d_result.reserve(res_bytes / sizeof(float)));
    if (int rc = h->upload(h->d_items, h->sched.items)) return rc;
    if (int rc = h->upload(h->d_oh, h->sched.oh_cols)) return rc;
    h->panel_cols = static_cast<int32_t>(L.C);
    SweepRun run;
    if (int rc = run.begin(*h, static_cast<double>(res_bytes))) return rc;
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_result, 0, res_bytes, h->stream));
    const int lpr = lanes_per_row(L.Cp / 2);
    auto launch = [&](const ListLaunch &l) {
        if (l.to_result)
            launch_step<true>(lpr, l.grid, h->stream, l.items, h->d_oh, l.n_items, h->slots<double>(), L.stride, L.Cp,
                              static_cast<int>(L.C), static_cast<int>(h->n_anc), l.panel0, h->d_result);
        else
            launch_step<false>(lpr, l.grid, h->stream, l.items, h->d_oh, l.n_items, h->slots<double>(), L.stride, L.Cp,
                               static_cast<int>(L.C), static_cast<int>(h->n_anc), l.panel0, h->d_result);
    };
    if (int rc = sweep_lists(run, h->sched, h->d_items, kGcPanels, L, h->n_anc, 4 * (64 / lpr), 1, launch)) return rc;
    return run.end(*h);
}

}  // namespace

extern "C" {

int genphi_gc_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                     const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, genphi_gc **out)
{
    if (out) *out = nullptr;
    if (int rc = check_create_args("genphi_gc_create", n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids, out, INT32_MAX)) return rc;
    return create_entry(out, "gen.gc", [&](genphi_gc *h) {
        h->panel_env = hook_count("GENPHI_GC_PANEL");
        h->group_env = hook_count("GENPHI_GC_PANELS_PER_LAUNCH");
        genphi::SweepOptions opt;
        opt.emit = genphi::Emit::LeafFirst;
        std::string err;
        const int rc = genphi::plan_sweep(h->sched, n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids, opt, err);
        if (rc) return genphi_set_error(rc, err);
        h->n_pro = n_pro; h->n_anc = n_anc;
        return GENPHI_OK;
    });
}

int genphi_gc_compute(genphi_gc *h, int32_t device) { return compute_entry(h, device, "genphi_gc_compute", "gen.gc", compute_impl); }

int genphi_gc_result_device(const genphi_gc *h, const float **d_ptr, int64_t *ld)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_result_device: nothing computed");
    put(d_ptr, h->d_result.get());
    put(ld, h->n_anc);
    return GENPHI_OK;
}

int genphi_gc_result_to_host(genphi_gc *h, float *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_result_to_host: nothing computed");
    if (h->empty()) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_result_to_host: out is NULL");
    return h->copy_out(out, h->d_result, h->result_bytes(), "gen.gc");
}

int genphi_gc_stats(const genphi_gc *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *panel_cols)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_stats: NULL handle");
    h->stats(sweep_ms, algorithmic_bytes, nullptr);
    put(peak_slots, h->sched.peak_slots);
    put(panel_cols, h->panel_cols);
    return GENPHI_OK;
}

void genphi_gc_destroy(genphi_gc *h) { destroy_entry(h); }

}  // extern "C"
