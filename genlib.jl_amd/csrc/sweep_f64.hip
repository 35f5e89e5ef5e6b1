// sweep_f64.hip -- the Float64-storage sweep (opts flag GENPHI_FLAG_STORAGE_F64: gen.f, genphi_phi_pairs and the Float64 result
// queries): its four kernels, its buffers and its launches.  genphi_compute_device (genphi_hip.hip) walks the same phases for both
// storage types and calls prepare_buffers64 / enqueue_sweep64 here where a Float32 sweep has its own; the launch geometry of the three
// level kernels is f64_geometry.h (host only, tests/f64_geometry_check.cpp).
//
// The sweep is eager: never captured into a graph (it leaves the Float32 sweep's eager / graph keys alone), calls no step hook and does
// not touch stay_active -- every level is written compactly, in the cut's storage order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "cut_format.h"
#include "f64_geometry.h"
#include "plan_device.h"

using genphi::kF64Cols;
using genphi::kF64Pre;
using genphi::kS64Cols;
using genphi::kS64Pre;

namespace {

using genphi::kOrdMask;      // (planner.h)

// ---- Float64 storage (opts flag GENPHI_FLAG_STORAGE_F64) -----------------------------------------
// The pairwise recursion of the reference, phi(i::Individual, j::Individual) (src/compute.jl:66-95),
// and gen.f built on it (:500-511) work in Float64 throughout and never round to Float32 between
// generations.  The same level sweep with Float64 level matrices reproduces them: every kinship
// is a dyadic rational, exactly representable in Float64 while the pedigree is less than ~26
// generations deep (then the sweep and the recursion are bit-identical whatever their order of
// operations).  Beyond, the four terms are grouped as the recursion groups them and scaled once
// (exact for normal doubles): bit-identical to the recursion memoised level by level (the oracle's
// Float64 sweep) wherever the result is normal, within 2 L 2^-53 relative of the exact kinship
// after L level steps; subnormal results are kept (no flush), within 4 x 2^-1074.  One thread per entry, four global gathers;
// meant for the small proband sets of gen.f / pairwise queries, not for throughput.
//   colmap: member index of output column j (the last level is delivered in proband order), or nullptr
__global__ void level_naive64_kernel(const double *__restrict__ psi, long long ld_prev, int n_prev, double *__restrict__ out,
                                     long long ld, int n, const int *__restrict__ srcA, const int *__restrict__ srcB,
                                     const int *__restrict__ ord, const int *__restrict__ rows, const int *__restrict__ out_rows,
                                     const int *__restrict__ colmap, int n_cols)
{
    const int w = blockIdx.x;
    const long long j = (long long)blockIdx.y * blockDim.x + threadIdx.x;
    if (j >= ld) return;
    const int i = rows ? rows[w] : w;
    const long long orow = out_rows ? out_rows[w] : i;
    double v = 0.0;
    if (j < n_cols) {
        const int jm = colmap ? colmap[j] : static_cast<int>(j);
        const int Ai = srcA[i], Bi = srcB[i], oi = ord[i];
        const int Aj = srcA[jm], Bj = srcB[jm], oj = ord[jm];
        const double *rowA = psi + (long long)Ai * ld_prev;
        const double *rowB = psi + (long long)Bi * ld_prev;
        if (jm == i && oi < 0) {
            v = 0.5 + 0.5 * rowA[Bi];
        } else {
            const double sc = (oi < 0 ? 0.5 : 1.0) * (oj < 0 ? 0.5 : 1.0);
            const double a = rowA[Aj], b = rowA[Bj], c = rowB[Aj], d = rowB[Bj];
            const bool i_hi = (oi & kOrdMask) > (oj & kOrdMask);
            const double x = i_hi ? b : c, y = i_hi ? c : b;
            v = ((a + x) + (y + d)) * sc;
        }
    }
    (void)n_prev; (void)n;
    out[orow * ld + j] = v;
}

// Float64 storage, cuts whose two source rows fit in LDS (2 x 8 bytes x (n_prev + 1) <= 160 KB): the FULL
// kernel's shape -- both source rows of an output row staged whole with 16-byte coalesced loads, four 8-byte LDS
// gathers per entry, coalesced row stores -- with the reference's grouping (src/compute.jl:66-95 climbs the
// higher-ranked individual first) and no rounding to Float32.  Same arguments as level_naive64_kernel + the number
// of rows.  PERSISTENT: a workgroup walks rows w = blockIdx.x, + gridDim.x, ... and
//   - owns the same columns in every row, so their index words (sources, rank word, member) are loaded ONCE into
//     registers (they were three dependent global loads per entry),
//   - has the NEXT row pair in flight into registers while the current one is gathered from LDS (rows of 7k+ members
//     leave room for one workgroup per CU only: nothing else would hide the load latency).
typedef double d2_t __attribute__((ext_vector_type(2)));   // (HIP's d2_t is a struct of unions: arrays of it stay in scratch)
__global__ void __launch_bounds__(512)
level_full64_kernel(const double *__restrict__ psi, long long ld_prev, int n_prev, double *__restrict__ out, long long ld,
                    const int *__restrict__ srcA, const int *__restrict__ srcB, const int *__restrict__ ord,
                    const int *__restrict__ rows, const int *__restrict__ out_rows, const int *__restrict__ colmap, int n_cols,
                    int lds_row, int n_rows)
{
    extern __shared__ double lds64[];
    double *sA = lds64, *sB = lds64 + lds_row;
    const int tid = threadIdx.x, nt = blockDim.x;
    unsigned pkj[kF64Cols];
    int oj[kF64Cols], jmv[kF64Cols];
    const int j0 = blockIdx.y * nt * kF64Cols;           // this workgroup's column chunk (outputs wider than 512 x 20 columns take several)
#pragma unroll
    for (int k = 0; k < kF64Cols; ++k) {
        const int j = j0 + tid + k * nt;
        pkj[k] = 0; oj[k] = 0; jmv[k] = -1;
        if (j < n_cols) {
            const int jm = colmap ? colmap[j] : j;
            jmv[k] = jm; pkj[k] = static_cast<unsigned>(srcA[jm]) | static_cast<unsigned>(srcB[jm]) << 16; oj[k] = ord[jm];
        }
    }
    const int nvec = lds_row >> 1;
    d2_t ra[kF64Pre], rb[kF64Pre];
#define GENPHI_F64_FETCH(W)                                                                                                    \
    {                                                                                                                          \
        const int fi = rows ? rows[W] : (W);                                                                                   \
        const d2_t *a2 = reinterpret_cast<const d2_t *>(psi + (long long)srcA[fi] * ld_prev);                            \
        const d2_t *b2 = reinterpret_cast<const d2_t *>(psi + (long long)srcB[fi] * ld_prev);  /* "none" = the zero row */ \
        _Pragma("unroll") for (int k = 0; k < kF64Pre; ++k) { const int q = min(tid + k * nt, nvec - 1); ra[k] = a2[q]; rb[k] = b2[q]; } \
    }
    int w = blockIdx.x;
    if (w >= n_rows) return;
    GENPHI_F64_FETCH(w)
    for (; w < n_rows; w += gridDim.x) {
        __syncthreads();                                  // the previous row's gathers are done
        {
            d2_t *sA2 = reinterpret_cast<d2_t *>(sA), *sB2 = reinterpret_cast<d2_t *>(sB);
#pragma unroll
            for (int k = 0; k < kF64Pre; ++k) { const int q = tid + k * nt; if (q < nvec) { sA2[q] = ra[k]; sB2[q] = rb[k]; } }
        }
        const int i = rows ? rows[w] : w;
        const long long orow = out_rows ? out_rows[w] : i;
        const int Bi = srcB[i], oi = ord[i];
        if (w + (int)gridDim.x < n_rows) GENPHI_F64_FETCH(w + (int)gridDim.x)      // in flight behind the gathers
        __syncthreads();
        const bool new_i = oi < 0;
        const int ord_i = oi & kOrdMask;
        double *orowp = out + orow * ld;
        unsigned z1 = 0;                                  // opaque zero: the LDS addresses of the 20 columns are row-invariant, and hipcc
        asm volatile("" : "+s"(z1));                      // would keep all 80 of them in registers across the row loop (spills)
#pragma unroll
        for (int k = 0; k < kF64Cols; ++k) {
            const int j = j0 + tid + k * nt;
            if (j >= ld) break;
            double v = 0.0;
            if (jmv[k] >= 0) {
                const unsigned pkz = pkj[k] ^ z1;
                const int ojz = oj[k] ^ static_cast<int>(z1);
                const unsigned Aj = pkz & 0xffffu, Bj = pkz >> 16;
                if (jmv[k] == i && new_i) {
                    v = 0.5 + 0.5 * sA[Bi];
                } else {
                    const double sc = (new_i ? 0.5 : 1.0) * (ojz < 0 ? 0.5 : 1.0);
                    const double a = sA[Aj], b = sA[Bj], c = sB[Aj], d = sB[Bj];
                    const bool i_hi = ord_i > (ojz & kOrdMask);
                    const double x = i_hi ? b : c, y = i_hi ? c : b;
                    v = ((a + x) + (y + d)) * sc;
                }
            }
            orowp[j] = v;
            if ((k & 1) == 1) __builtin_amdgcn_sched_barrier(0);      // two columns' gathers in flight, not twenty (registers)
        }
    }
    (void)n_prev;
#undef GENPHI_F64_FETCH
}

// Float64 storage, cuts whose rows fit in LDS one at a time (8 bytes x (n_prev + 1) <= 160 KB: up to 20,479 members): the SPLIT
// kernels' shape in its simplest form.  A workgroup walks a contiguous piece of the row list (rows sharing the A source are
// adjacent in a step's work order) for one chunk of 512 x 14 columns: row A is staged and its terms (a, b) of the chunk's columns
// kept in registers for as long as the following rows share it; every row with a B source stages that row, gathers (c, d), combines
// with the reference's grouping and stores.  The next row to stage is in flight into registers behind the gathers.  Same arguments
// as level_full64_kernel.
__global__ void __launch_bounds__(512)
level_split64_kernel(const double *__restrict__ psi, long long ld_prev, int n_prev, double *__restrict__ out, long long ld,
                     const int *__restrict__ srcA, const int *__restrict__ srcB, const int *__restrict__ ord,
                     const int *__restrict__ rows, const int *__restrict__ out_rows, const int *__restrict__ colmap, int n_cols,
                     int lds_row, int n_rows)
{
    extern __shared__ double srow[];
    const int tid = threadIdx.x;
    constexpr int nt = 512;
    unsigned pkj[kS64Cols];
    int oj[kS64Cols], jmv[kS64Cols];
    double va[kS64Cols], vb[kS64Cols];
    const int j0 = blockIdx.y * nt * kS64Cols;
#pragma unroll
    for (int k = 0; k < kS64Cols; ++k) {
        const int j = j0 + tid + k * nt;
        pkj[k] = 0; oj[k] = 0; jmv[k] = -1; va[k] = vb[k] = 0.0;
        if (j < n_cols) {
            const int jm = colmap ? colmap[j] : j;
            jmv[k] = jm; pkj[k] = static_cast<unsigned>(srcA[jm]) | static_cast<unsigned>(srcB[jm]) << 16; oj[k] = ord[jm];
        }
    }
    const int per = (n_rows + static_cast<int>(gridDim.x) - 1) / static_cast<int>(gridDim.x);
    const int w0 = blockIdx.x * per, w1 = min(n_rows, w0 + per);
    if (w0 >= w1) return;
    const int nvec = lds_row >> 1;
    d2_t pre[kS64Pre];
    auto fetch = [&](int r) {
        const d2_t *g2 = reinterpret_cast<const d2_t *>(psi + (long long)r * ld_prev);
#pragma unroll
        for (int k = 0; k < kS64Pre; ++k) pre[k] = g2[min(tid + k * nt, nvec - 1)];
    };
    auto to_lds = [&]() {
        __syncthreads();                                  // the gathers from the previous row are done
        d2_t *s2 = reinterpret_cast<d2_t *>(srow);
#pragma unroll
        for (int k = 0; k < kS64Pre; ++k) { const int q = tid + k * nt; if (q < nvec) s2[q] = pre[k]; }
        __syncthreads();
    };
    // the row staged after (w, A just staged?): B of w, else the first A change / B source of the following rows; -1: none left
    auto next_stage = [&](int w, bool after_a, int cur_a) -> int {
        if (after_a) { const int b = srcB[rows ? rows[w] : w]; if (b != n_prev) return b; }
        for (int v = w + 1; v < w1; ++v) {
            const int i2 = rows ? rows[v] : v;
            if (srcA[i2] != cur_a) return srcA[i2];
            if (srcB[i2] != n_prev) return srcB[i2];
        }
        return -1;
    };
    int cur_a = -1;
    {
        const int i0 = rows ? rows[w0] : w0;
        fetch(srcA[i0]);                                  // ("none" is the all-zero row: a parentless member's A)
    }
    for (int w = w0; w < w1; ++w) {
        const int i = rows ? rows[w] : w;
        const long long orow = out_rows ? out_rows[w] : i;
        const int Ai = srcA[i], Bi = srcB[i], oi = ord[i];
        const bool new_i = oi < 0;
        const int ord_i = oi & kOrdMask;
        unsigned z1 = 0;                                  // opaque zero (see level_full64_kernel)
        asm volatile("" : "+s"(z1));
        if (Ai != cur_a) {                                // stage A, keep its terms
            to_lds();
            cur_a = Ai;
            const int nx = next_stage(w, true, cur_a);
            if (nx >= 0) fetch(nx);
#pragma unroll
            for (int k = 0; k < kS64Cols; ++k) {
                const unsigned pkz = pkj[k] ^ z1;
                va[k] = srow[pkz & 0xffffu]; vb[k] = srow[pkz >> 16];
            }
        }
        const bool has_b = Bi != n_prev;
        if (has_b) {
            to_lds();                                     // row B
            const int nx = next_stage(w, false, cur_a);
            if (nx >= 0) fetch(nx);
        }
        double *orowp = out + orow * ld;
#pragma unroll
        for (int k = 0; k < kS64Cols; ++k) {
            const int j = j0 + tid + k * nt;
            if (j >= ld) break;
            double v = 0.0;
            if (jmv[k] >= 0) {
                const unsigned pkz = pkj[k] ^ z1;
                const int ojz = oj[k] ^ static_cast<int>(z1);
                if (jmv[k] == i && new_i) {
                    v = 0.5 + 0.5 * (has_b ? srow[Ai] : 0.0);     // Psi[B][A] = Psi[A][B] (bit-symmetric levels)
                } else {
                    const double sc = (new_i ? 0.5 : 1.0) * (ojz < 0 ? 0.5 : 1.0);
                    const double a = va[k], b = vb[k];
                    const double c = has_b ? srow[pkz & 0xffffu] : 0.0, d = has_b ? srow[pkz >> 16] : 0.0;
                    const bool i_hi = ord_i > (ojz & kOrdMask);
                    const double x = i_hi ? b : c, y = i_hi ? c : b;
                    v = ((a + x) + (y + d)) * sc;
                }
            }
            orowp[j] = v;
            if ((k & 1) == 1) __builtin_amdgcn_sched_barrier(0);
        }
    }
}

__global__ void half_identity64_kernel(double *m, long long ld, int n, const int *out_rows, int n_rows, const int *colmap)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_rows) return;
    // row k of the output is member (colmap ? colmap[k'] ...): used only for the all-founders case,
    // where every member is a proband: diagonal of the delivered matrix
    (void)colmap; (void)out_rows; (void)n;
    m[(long long)k * ld + k] = 0.5;
}
}  // namespace

// Everything a Float64 sweep writes to: the result, the rows of the shard, timing events, sparse levels, the Float64 level buffers
int prepare_buffers64(genphi_plan *p, SweepCall &c, bool no_sparse, PhaseTrace &trace)
{
    const Plan &pl = p->plan;
    const int L = pl.n_levels, n_steps = L - 1;
    const int64_t ldN = pl.ld[L - 1], r0 = c.r0, n_rows = c.n_rows;
    p->res_ld = ldN;
    HIP_TRY_AS("genphi::cached_malloc(reinterpret_cast<void **>(ptr), std::max<size_t>(need, 1) * sizeof(double))", p->result64.reserve(static_cast<size_t>(n_rows * ldN)));
    // storage member of each resident row (the last cut may be stored in [dragged, new] order)
    std::vector<int> srow(n_rows), orow(n_rows);
    for (int64_t k = 0; k < n_rows; ++k) { srow[k] = pl.final_perm.empty() ? static_cast<int>(r0 + k) : pl.final_perm[r0 + k]; orow[k] = static_cast<int>(k); }
    HIP_TRY_AS("genphi::cached_malloc(reinterpret_cast<void **>(&p->d_perm_rows), 2 * n_rows * sizeof(int))", p->d_perm_rows.reserve(static_cast<size_t>(2 * n_rows)));
    HIP_TRY(hipMemcpyAsync(p->d_perm_rows, srow.data(), n_rows * sizeof(int), hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipMemcpyAsync(p->d_perm_rows + n_rows, orow.data(), n_rows * sizeof(int), hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));           // host vectors go out of scope
    if (n_steps == 0) { c.timing = false; return GENPHI_OK; }      // (no level to time: the stats of such a call have never been `timed`)
    int rc;
    if (c.timing) {
        rc = ensure_events(p, n_steps + 3);
        if (rc) return rc;
    }
    // the leading cuts as lists of their non-zero entries here too (integer values are exact for Float64 as for Float32, sparse_levels.h):
    // the first dense matrix is written in Float64, compactly
    rc = ensure_sparse_levels(p, c.kernel, trace);
    if (rc) return rc;
    c.sparse_k = (c.kernel == 0 && p->sparse && !no_sparse) ? genphi::sparse_levels_k(p->sparse) : -1;
    // Float64 level matrices of the cuts that exist as matrices (cuts 0..sparse_k live as row lists): genea140 2 x 1.5 GB -> 2 x 0.2
    size_t need[2] = {0, 0};
    for (int k = c.sparse_k + 1; k + 1 < L; ++k) need[k & 1] = std::max(need[k & 1], static_cast<size_t>((pl.cut_sizes[k] + 1) * pl.ld[k]));
    for (int b = 0; b < 2; ++b)
        if (need[b]) HIP_TRY_AS("genphi::cached_malloc(reinterpret_cast<void **>(ptr), std::max<size_t>(need, 1) * sizeof(double))", p->buf64[b].reserve(need[b]));
    return GENPHI_OK;
}

// Level step s > c.sparse_k: cut s (buf64[s & 1]) -> cut s + 1, or, the last step, the shard's rows of the result in proband order
static int launch_level64(genphi_plan *p, const SweepCall &c, int s)
{
    const Plan &pl = p->plan;
    const LevelStep &st = pl.steps[s];
    const DeviceStep &d = p->dsteps[s];
    const int64_t n_rows = c.n_rows;
    const double *psi = p->buf64[s & 1];
    const bool last = s == pl.n_levels - 2;
    double *out = last ? p->result64 : p->buf64[(s + 1) & 1];
    const int rows_n = last ? static_cast<int>(n_rows) : static_cast<int>(st.n);
    const int *k_rows = last ? p->d_perm_rows : static_cast<const int *>(nullptr);
    const int *k_orows = last ? p->d_perm_rows + n_rows : static_cast<const int *>(nullptr);
    const int *k_colmap = (last && !pl.final_perm.empty()) ? p->d_final_perm : static_cast<const int *>(nullptr);
    const genphi::F64Geometry g = genphi::f64_geometry(st.n_prev, st.ld, rows_n, p->n_cus, c.kernel, genphi::f64_lds_budget(p->tun.lds_cap_floats));
    const dim3 grid(static_cast<unsigned>(g.grid_x), static_cast<unsigned>(g.grid_y)), block(static_cast<unsigned>(g.block));
    if (g.form == genphi::kF64Full) {
        const size_t lds64 = g.lds_bytes;
        HIP_TRY(set_max_lds(reinterpret_cast<const void *>(level_full64_kernel), lds64));
        hipLaunchKernelGGL(level_full64_kernel, grid, block, lds64, p->stream, psi,
                           static_cast<long long>(st.ld_prev), static_cast<int>(st.n_prev), out, static_cast<long long>(st.ld), d.srcA, d.srcB,
                           d.ord, k_rows, k_orows, k_colmap, static_cast<int>(st.n), g.lds_row, rows_n);
    } else if (g.form == genphi::kF64Split) {
        // rows in the step's work order (same A source adjacent) where the step has one
        const size_t lds1 = g.lds_bytes;
        HIP_TRY(set_max_lds(reinterpret_cast<const void *>(level_split64_kernel), lds1));
        const int *w_rows = last ? k_rows : ((st.mode != genphi::kModeWide && static_cast<int64_t>(st.work.size()) == st.n) ? d.work : static_cast<const int *>(nullptr));
        hipLaunchKernelGGL(level_split64_kernel, grid, block, lds1, p->stream, psi,
                           static_cast<long long>(st.ld_prev), static_cast<int>(st.n_prev), out, static_cast<long long>(st.ld), d.srcA, d.srcB,
                           d.ord, w_rows, k_orows, k_colmap, static_cast<int>(st.n), g.lds_row, rows_n);
    } else {
        hipLaunchKernelGGL(level_naive64_kernel, grid, block, 0, p->stream, psi, static_cast<long long>(st.ld_prev),
                           static_cast<int>(st.n_prev), out, static_cast<long long>(st.ld), static_cast<int>(st.n), d.srcA, d.srcB, d.ord,
                           k_rows, k_orows, k_colmap, static_cast<int>(st.n));
    }
    HIP_TRY(hipGetLastError());
    if (!last)           // the all-zero "none" row of this level
        HIP_TRY(hipMemsetAsync(out + st.n * st.ld, 0, static_cast<size_t>(st.ld) * sizeof(double), p->stream));
    if (c.timing) HIP_TRY(hipEventRecord(p->events[s + 1], p->stream));
    return GENPHI_OK;
}

// The whole sweep with Float64 level matrices (see level_naive64_kernel), in stream order: rows [r0, r0 + n_rows) of the proband matrix
// end up in p->result64 (row pitch = pitch of the last cut)
int enqueue_sweep64(genphi_plan *p, const SweepCall &c)
{
    const Plan &pl = p->plan;
    const int n_steps = pl.n_levels - 1;
    if (n_steps == 0) {
        // all probands parentless: 1/2 I (src/compute.jl:271-274, loop skipped); members = probands in order, so row k of the shard has
        // its diagonal entry in column r0 + k
        const int64_t ldN = pl.ld[0], n_rows = c.n_rows;
        HIP_TRY(hipMemsetAsync(p->result64, 0, static_cast<size_t>(n_rows * ldN) * sizeof(double), p->stream));
        hipLaunchKernelGGL(half_identity64_kernel, dim3(static_cast<unsigned>((n_rows + 255) / 256)), dim3(256), 0, p->stream, p->result64 + c.r0,
                           static_cast<long long>(ldN), static_cast<int>(n_rows), static_cast<const int *>(nullptr), static_cast<int>(n_rows),
                           static_cast<const int *>(nullptr));
        HIP_TRY(hipGetLastError());
        return GENPHI_OK;
    }
    if (c.sparse_k < 0) {
        const int64_t n0 = pl.cut_sizes[0], ld0 = pl.ld[0];
        HIP_TRY(hipMemsetAsync(p->buf64[0], 0, static_cast<size_t>((n0 + 1) * ld0) * sizeof(double), p->stream));
        hipLaunchKernelGGL(half_identity64_kernel, dim3(static_cast<unsigned>((n0 + 255) / 256)), dim3(256), 0, p->stream, p->buf64[0],
                           static_cast<long long>(ld0), static_cast<int>(n0), static_cast<const int *>(nullptr), static_cast<int>(n0),
                           static_cast<const int *>(nullptr));
        HIP_TRY(hipGetLastError());
    }
    for (int s = 0; s < n_steps; ++s) {
        const int rc = s <= c.sparse_k ? enqueue_list_step(p, c, s, p->buf64[(s + 1) & 1], true, genphi::kFmtF32, nullptr) : launch_level64(p, c, s);
        if (rc) return rc;
    }
    return GENPHI_OK;
}
