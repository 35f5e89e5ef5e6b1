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

#include "sweep_device.h"

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

// 16-bit rows, 8 columns per 16 bytes; default panels (sweep_panels.h) of at least 64 columns, a multiple of 8 (16-byte result
// stores) and never narrower than 8
constexpr int64_t kVec = 8;
constexpr genphi::PanelRule kDistPanels = {2, 1, kVec, 64, kVec, kVec, kVec};

}  // namespace

struct genphi_dist : SweepDevice {
    int64_t n_pro = 0, n_anc = 0, ld = 0;
    genphi::SweepSchedule sched;             // host schedule (ancestor_sweep.h)
    int32_t panel_env = 0, group_env = 0;    // GENPHI_DIST_PANEL / GENPHI_DIST_PANELS_PER_LAUNCH (0 = default rule)
    DevBuf<short> d_result;                  // n_pro rows of ld entries
    DevBuf<int4> d_items;
    DevBuf<int> d_oh;
    int32_t panel_cols = 0;
    genphi_dist() { own(d_result, d_items, d_oh); }
    size_t result_bytes() const { return static_cast<size_t>(n_pro) * static_cast<size_t>(ld) * sizeof(short); }
    bool empty() const { return n_anc == 0 || n_pro == 0; }
};

namespace {

void launch_list(genphi_dist *h, int lpr, const ListLaunch &l, bool aligned, const genphi::PanelLayout &L)
{
    unsigned short *slots = h->slots<unsigned short>();
    const int n_anc = static_cast<int>(h->n_anc), C = static_cast<int>(L.C);
    if (!l.to_result) {
        GENPHI_LPR_SWITCH(lpr, (dist_step_kernel<LPR, false, false><<<l.grid, 256, 0, h->stream>>>(l.items, h->d_oh, l.n_items, slots, L.stride, L.Cp,
                                                                                                  C, n_anc, l.panel0, nullptr, 0)));
    } else if (aligned) {
        GENPHI_LPR_SWITCH(lpr, (dist_step_kernel<LPR, true, true><<<l.grid, 256, 0, h->stream>>>(l.items, h->d_oh, l.n_items, slots, L.stride, L.Cp,
                                                                                                C, n_anc, l.panel0, h->d_result, h->ld)));
    } else {
        GENPHI_LPR_SWITCH(lpr, (dist_step_kernel<LPR, true, false><<<l.grid, 256, 0, h->stream>>>(l.items, h->d_oh, l.n_items, slots, L.stride, L.Cp,
                                                                                                 C, n_anc, l.panel0, h->d_result, h->ld)));
    }
}

int compute_impl(genphi_dist *h, int32_t device)
{
    if (int rc = h->select(device)) return rc;
    const size_t res_bytes = h->result_bytes();
    genphi::PanelLayout L;
    if (int rc = h->size_panels(L, kDistPanels, h->sched, h->n_anc, h->panel_env, h->group_env, res_bytes, h->d_result.get() != nullptr, "gen.meioses"))
        return rc;
    GENPHI_HIP_TRY(h->d_result.reserve(res_bytes / sizeof(short)));
    if (int rc = h->upload(h->d_items, h->sched.items)) return rc;
    if (int rc = h->upload(h->d_oh, h->sched.oh_cols)) return rc;
    h->panel_cols = static_cast<int32_t>(L.C);
    SweepRun run;
    if (int rc = run.begin(*h, static_cast<double>(h->n_pro) * static_cast<double>(h->n_anc) * sizeof(short))) return rc;
    // -1 everywhere: the probands whose row is "none" are not in the last list
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_result, 0xFF, res_bytes, h->stream));
    const int lpr = lanes_per_row(static_cast<int>(L.Cp / kVec));
    const bool aligned = L.C % kVec == 0 || L.n_panels == 1;      // every panel starts on a multiple of 8 columns
    if (int rc = sweep_lists(run, h->sched, h->d_items, kDistPanels, L, h->n_anc, 4 * (64 / lpr), 1,
                             [&](const ListLaunch &l) { launch_list(h, lpr, l, aligned, L); }))
        return rc;
    return run.end(*h);
}

}  // namespace

extern "C" {

int genphi_dist_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                       const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, genphi_dist **out)
{
    if (out) *out = nullptr;
    if (int rc = check_create_args("genphi_dist_create", n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids, out, INT32_MAX - 64)) return rc;
    return create_entry(out, "gen.meioses", [&](genphi_dist *h) {
        h->panel_env = hook_count("GENPHI_DIST_PANEL");
        h->group_env = hook_count("GENPHI_DIST_PANELS_PER_LAUNCH");
        genphi::SweepOptions opt;
        opt.emit = genphi::Emit::EveryProband;
        opt.first_onehot_only = false;
        opt.mark_copies = true;
        std::string err;
        if (const int rc = genphi::plan_sweep(h->sched, n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids, opt, err)) return genphi_set_error(rc, err);
        if (h->sched.n_steps > GENPHI_DIST_MAX_STEPS)
            return genphi_set_error(GENPHI_ERR_ARG, "gen.meioses: a sweep of " + std::to_string(h->sched.n_steps) + " steps; the signed 16-bit result holds at most " +
                                                        std::to_string(GENPHI_DIST_MAX_STEPS) + " meioses");
        h->n_pro = h->sched.n_pro; h->n_anc = n_anc;
        h->ld = (n_anc + kVec - 1) / kVec * kVec;
        return GENPHI_OK;
    });
}

int genphi_dist_compute(genphi_dist *h, int32_t device) { return compute_entry(h, device, "genphi_dist_compute", "gen.meioses", compute_impl); }

int genphi_dist_result_device(const genphi_dist *h, const int16_t **d_ptr, int64_t *ld)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_dist_result_device: nothing computed");
    put(d_ptr, h->d_result.get());
    put(ld, h->ld);
    return GENPHI_OK;
}

int genphi_dist_result_to_host(genphi_dist *h, int16_t *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_dist_result_to_host: nothing computed");
    if (h->empty()) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_dist_result_to_host: out is NULL");
    const size_t width = static_cast<size_t>(h->n_anc) * sizeof(short);
    return h->copy_out_2d(out, h->d_result, static_cast<size_t>(h->ld) * sizeof(short), width, static_cast<size_t>(h->n_pro), "gen.meioses");
}

int genphi_dist_stats(const genphi_dist *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *panel_cols,
                      int32_t *row_bits, int64_t *launches)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_dist_stats: NULL handle");
    h->stats(sweep_ms, algorithmic_bytes, launches);
    put(peak_slots, h->sched.peak_slots);
    put(panel_cols, h->panel_cols);
    put(row_bits, 16);
    return GENPHI_OK;
}

void genphi_dist_destroy(genphi_dist *h) { destroy_entry(h); }

}  // extern "C"
