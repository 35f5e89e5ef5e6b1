// label_sweep.h -- the label sweep that gen.simuIdentity, gen.simuRetention and gen.simuSharing share (ident.hip, retain.hip, link.hip):
// every founder allele is dropped under its own label of B bits (the plan is ident.h's).  A panel row holds Cn columns of 16-byte
// elements: row r, column c, side s, plane b at ((r * Cn + c) * 2 + s) * B + b.  ident and retain: a column is a pair of words of the
// simulations; link: a pair of words of the loci of one simulation.  Here:
//   kernels  init (the constant sides) and gather (the listed probands' rows, transposed) for any columns; the step kernel of one
//            level on ident's columns (link.hip keeps its own, over (simulation, locus))
//   handle   LabelSweep, the base of genphi_ident, genphi_retain and genphi_link: the plan, S, the seed, the lists on the device and
//            the launches above
//   entries  the bodies of genphi_*_alleles and genphi_*_labels_to_host
// Every including file gets its own copy (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>

#include "drop_device.h"
#include "drop_host.h"
#include "ident.h"

namespace {

// The constant sides: a thread per (label, column) writes the B planes of the side that carries the label.
__global__ void __launch_bounds__(256)
label_init_kernel(const long long *__restrict__ const_side, long long n_labels, ulonglong2 *__restrict__ rows, long long Cn, long long Cc, int B)
{
    const long long t = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const long long k = t / Cc;
    if (k >= n_labels) return;
    const long long c = t % Cc;
    const long long side = const_side[k];                // 2 * row + side
    ulonglong2 *dst = rows + ((side >> 1) * Cn + c) * 2 * B + (side & 1) * B;
    for (int b = 0; b < B; ++b) {
        const u64 v = (k >> b) & 1 ? ~0ull : 0ull;
        dst[b] = make_ulonglong2(v, v);
    }
}

// One level: row row0 + r from the rows of its parents (simu_step_kernel's lanes: LPR lanes per row, lane l owns the pairs l,
// l + LPR, .. < Pc; a wave holds 64 / LPR rows).  A parent row < 0 is a constant side: the init kernel wrote it.  rows is read
// (earlier levels) and written (this level): no __restrict__.
template <int LPR>
__global__ void __launch_bounds__(256)
ident_step_kernel(const int *__restrict__ fa_row, const int *__restrict__ mo_row, const long long *__restrict__ ids, int n_rows,
                  long long row0, ulonglong2 *rows, int Pn, int Pc, int B, unsigned first_pair, unsigned k0, unsigned k1)
{
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = (static_cast<long long>(blockIdx.x) * 4 + wave) * RPW + lane / LPR;
    if (r >= n_rows) return;
    const int l = lane % LPR;
    const int f = fa_row[r], m = mo_row[r];
    const u64 id = static_cast<u64>(ids[r]);
    const unsigned id_lo = static_cast<unsigned>(id), id_hi = static_cast<unsigned>(id >> 32);
    const long long B2 = 2 * B;
    const ulonglong2 *fs = rows + static_cast<long long>(f < 0 ? 0 : f) * Pn * B2;
    const ulonglong2 *ms = rows + static_cast<long long>(m < 0 ? 0 : m) * Pn * B2;
    ulonglong2 *dst = rows + (row0 + r) * Pn * B2;
    for (int c = l; c < Pc; c += LPR) {
        if (f >= 0) {
            const ulonglong2 T = philox_pair(id_lo, id_hi, first_pair + static_cast<unsigned>(c), 0u, k0, k1);
            const ulonglong2 *src = fs + c * B2;
            ulonglong2 *out = dst + c * B2;
            for (int b = 0; b < B; ++b) {
                const ulonglong2 p = src[b], q = src[B + b];
                out[b] = meiosis(T, p, q);
            }
        }
        if (m >= 0) {
            const ulonglong2 T = philox_pair(id_lo, id_hi, first_pair + static_cast<unsigned>(c), 1u, k0, k1);
            const ulonglong2 *src = ms + c * B2;
            ulonglong2 *out = dst + c * B2 + B;
            for (int b = 0; b < B; ++b) {
                const ulonglong2 p = src[b], q = src[B + b];
                out[b] = meiosis(T, p, q);
            }
        }
    }
}

// The listed probands' rows, transposed: column c, side s, plane b, proband i at ((c * 2 + s) * B + b) * n_pro + i.  Consecutive
// threads own consecutive probands of one (column, side, plane).
__global__ void __launch_bounds__(256)
label_gather_kernel(const ulonglong2 *__restrict__ rows, const int *__restrict__ pro_row, int n_pro, long long Cn, long long Cc, int B2,
                    ulonglong2 *__restrict__ gathered)
{
    const long long t = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const int i = static_cast<int>(t % n_pro);
    const long long e = t / n_pro;                       // column * B2 + (side * B + plane)
    if (e >= Cc * B2) return;
    const long long c = e / B2, k = e % B2;
    gathered[e * n_pro + i] = rows[(static_cast<long long>(pro_row[i]) * Cn + c) * B2 + k];
}

// What the three handles hold alike; d_slots: the rows of one panel.  A handle adds its results and registers them (own) itself.
struct LabelSweep : SweepDevice {
    genphi::IdentPlan plan;                  // host plan (ident.h)
    int64_t S = 0;
    uint64_t seed = 0;
    int32_t panel_arg = 0;                   // create's panel_cols / panel_sims (0 = default rule)
    DevBuf<int> d_fa, d_mo, d_pro_row;
    DevBuf<long long> d_ids, d_const_side;
    LabelSweep() { own(d_fa, d_mo, d_pro_row, d_ids, d_const_side); }
    bool empty() const { return false; }     // (n_pro >= 1 and S >= 1 always)

    // the lists of the plan, uploaded once (ident.h: label_list_bytes)
    int upload_lists()
    {
        int rc;
        if ((rc = upload(d_fa, plan.fa_row)) || (rc = upload(d_mo, plan.mo_row)) || (rc = upload(d_pro_row, plan.pro_row)) ||
            (rc = upload(d_ids, plan.row_id)) || (rc = upload(d_const_side, plan.const_side)))
            return rc;
        return GENPHI_OK;
    }

    // init: the first Cc columns of the panel's Cn
    int init_panel(long long Cn, long long Cc)
    {
        label_init_kernel<<<static_cast<unsigned>((plan.n_labels * Cc + 255) / 256), 256, 0, stream>>>(d_const_side.get(), plan.n_labels, slots<ulonglong2>(), Cn,
                                                                                                        Cc, plan.planes);
        GENPHI_HIP_TRY(hipGetLastError());
        return GENPHI_OK;
    }

    // gather: the first Cc columns of the listed probands' rows
    int gather_panel(long long Cn, long long Cc, ulonglong2 *gathered)
    {
        const long long threads = static_cast<long long>(plan.n_pro) * Cc * 2 * plan.planes;
        label_gather_kernel<<<static_cast<unsigned>((threads + 255) / 256), 256, 0, stream>>>(slots<ulonglong2>(), d_pro_row.get(), static_cast<int>(plan.n_pro), Cn,
                                                                                              Cc, 2 * plan.planes, gathered);
        GENPHI_HIP_TRY(hipGetLastError());
        return GENPHI_OK;
    }
};

// The label sweep of one panel on ident's columns (h->panels): init, then one launch per level >= 1.  Pc pairs from the absolute pair
// first_pair.  A template, so that only a file that calls it carries the step kernels.
template <typename H>
int label_sweep_panel(H *h, int Pc, unsigned first_pair)
{
    const genphi::IdentPlan &pl = h->plan;
    const int Pn = h->panels.pairs, lpr = h->panels.lanes_per_row, B = pl.planes, step_rows = 4 * (64 / lpr);
    const unsigned k0 = static_cast<unsigned>(h->seed), k1 = static_cast<unsigned>(h->seed >> 32);
    ulonglong2 *rows = h->template slots<ulonglong2>();
    if (int rc = h->init_panel(Pn, Pc)) return rc;
    for (int k = 1; k < pl.n_levels; ++k) {
        const long long b = pl.level_begin[k];
        const int n_rows = static_cast<int>(pl.level_rows[k]);
        const unsigned grid = static_cast<unsigned>((n_rows + step_rows - 1) / step_rows);
        GENPHI_LPR_SWITCH(lpr, (ident_step_kernel<LPR><<<grid, 256, 0, h->stream>>>(h->d_fa.get() + b, h->d_mo.get() + b, h->d_ids.get() + b, n_rows, b, rows,
                                                                                 Pn, Pc, B, first_pair, k0, k1)));
        GENPHI_HIP_TRY(hipGetLastError());
    }
    return GENPHI_OK;
}

// The body of genphi_*_alleles; fn: the entry point's name.
inline int label_alleles(const LabelSweep *h, const char *fn, int64_t *n_labels, int32_t *planes, int64_t *ids, int32_t *sides)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, std::string(fn) + ": NULL handle");
    put(n_labels, h->plan.n_labels);
    put(planes, h->plan.planes);
    if (ids) std::copy(h->plan.allele_id.begin(), h->plan.allele_id.end(), ids);
    if (sides) std::copy(h->plan.allele_side.begin(), h->plan.allele_side.end(), sides);
    return GENPHI_OK;
}

// The body of genphi_*_labels_to_host for a handle with want_labels and d_labels; flag: the create flag's name.
template <typename H>
int labels_to_host(H *h, int32_t *out, const char *fn, const char *flag, const char *who)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, std::string(fn) + ": NULL handle");
    if (!h->want_labels) return genphi_set_error(GENPHI_ERR_ARG, std::string(fn) + ": the handle was created without " + flag);
    return result_to_host(h, out, &H::d_labels, fn, who);
}

}  // namespace
