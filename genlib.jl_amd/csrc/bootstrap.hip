// bootstrap.hip -- gen.phiCI on the resident kinship matrix (include/genphi.h, genphi_result_bootstrap).
//
// b bootstrap resamples of the N probands: with c_r[i] the number of times resample r drew proband i,
//     quad[r] = sum over the resident rows i and all columns j of c_r[i] c_r[j] Phi[i][j],    self[r] = sum_i c_r[i] Phi[i][i],
// that is the diagonal of C' Phi C for the N x b matrix C of counts: a Float64 matrix product fused with its own reduction.
// Resamples are worked off in panels of P; per panel three kernels on one stream:
//   counts   one workgroup per resample: the N draws (bootstrap.h: one Philox block per two draws) as Int32 atomic adds into
//            counts[j][r] (zeroed before), column-major in the resamples: the tile the product stages is then contiguous.  Int32
//            holds any count <= N < 2^31; integer adds commute, so the table does not depend on the order of the atomics
//   quad     a workgroup of 256 threads owns BR resident rows x PT resamples.  It walks the columns in chunks of KC: the Phi
//            tile (BR x KC, 16-byte loads, transposed into LDS as Float64) and the counts tile (KC x PT, Int32 -> Float64), the
//            next chunk's loads in flight in registers while this one is multiplied; Y = Phi C stays in a TR x TP register tile
//            per thread, accumulated by fma (c_j Phi_ij is exact in Float64).  At the end of the row block c_i Y_i and
//            c_i Phi_ii are folded over the thread's rows, then over the 16 thread rows through LDS in a fixed order: one partial
//            per (row block, resample), no floating-point atomics
//   reduce   a thread per resample adds the partials of the row blocks in block order
// The summation order of a resample depends on (N, the resident rows) alone: not on the panel width, on b or on
// `first`.  Padding: the counts table has a multiple of 64 rows and a multiple of 128 columns, all zero beyond N and P; the result's
// padding columns are zero (and multiply zero counts); rows beyond the resident ones are never read.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bootstrap.h"

namespace genphi {
namespace {

constexpr int kBootThreads = 256;
constexpr int kBootTR = 8, kBootTP = 8, kBootKC = 16;      // the product's tile: 128 rows x 128 resamples per workgroup, chunks of 16 columns
constexpr int kBootRows = 16 * kBootTR;
constexpr int kBootPad = 16 * kBootTP;         // the resample stride of a panel's tables is a multiple of the tile's width
constexpr int kBootMaxPanel = 8192;
constexpr size_t kBootCountsBudget = size_t(256) << 20;     // bytes of a panel's counts table under the default rule

size_t al256(size_t b) { return (b + 255) / 256 * 256; }
int round_up(int v, int m) { return (v + m - 1) / m * m; }

__global__ __launch_bounds__(kBootThreads) void boot_counts_kernel(int *__restrict__ counts, int pstride, int n, unsigned long long seed, unsigned first)
{
    const unsigned r = first + blockIdx.x;
    const unsigned pairs = (static_cast<unsigned>(n) + 1u) >> 1;
    for (unsigned pair = threadIdx.x; pair < pairs; pair += kBootThreads) {
        const BootDraws d = boot_draws(static_cast<uint64_t>(n), seed, r, pair);
        atomicAdd(counts + static_cast<size_t>(d.s0) * pstride + blockIdx.x, 1);
        if (2u * pair + 1u < static_cast<unsigned>(n)) atomicAdd(counts + static_cast<size_t>(d.s1) * pstride + blockIdx.x, 1);
    }
}

// grid (row blocks, resample tiles).  part_quad / part_self: [row block][pstride]
template <int TR, int TP, int KC>
__global__ __launch_bounds__(kBootThreads) void boot_quad_kernel(const float *__restrict__ phi, long long ld, int n, int row_begin, int n_rows,
                                                                 const int *__restrict__ counts, int pstride,
                                                                 double *__restrict__ part_quad, double *__restrict__ part_self)
{
    constexpr int BR = 16 * TR, PT = 16 * TP, LDA = BR + 2;
    constexpr int QA = KC / 4, QC = PT / 4;                              // quads per row of the Phi tile / of the counts tile
    constexpr int NA = BR * QA / kBootThreads, NC = KC * QC / kBootThreads;
    static_assert(BR * QA % kBootThreads == 0 && KC * QC % kBootThreads == 0 && KC % 4 == 0 && 64 % KC == 0, "tile shapes");
    static_assert(KC >= 16, "the fold reuses the counts tile as 16 x PT partials");
    __shared__ double sA[KC][LDA];         // Phi tile, transposed: [column][row]
    __shared__ double sC[KC][PT];          // counts tile: [column][resample]
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int k0 = blockIdx.x * BR, p0 = blockIdx.y * PT;
    const int chunks = (n + KC - 1) / KC;

    float4 ra[NA];
    int4 rc[NC];
    auto load = [&](int j0) {
#pragma unroll
        for (int u = 0; u < NA; ++u) {
            const int idx = tid + u * kBootThreads, i = idx / QA, q = idx % QA;
            ra[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k0 + i < n_rows) ra[u] = *reinterpret_cast<const float4 *>(phi + static_cast<long long>(k0 + i) * ld + j0 + 4 * q);
        }
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            const int idx = tid + u * kBootThreads, j = idx / QC, q = idx % QC;
            rc[u] = *reinterpret_cast<const int4 *>(counts + static_cast<size_t>(j0 + j) * pstride + p0 + 4 * q);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int u = 0; u < NA; ++u) {
            const int idx = tid + u * kBootThreads, i = idx / QA, q = idx % QA;
            sA[4 * q + 0][i] = static_cast<double>(ra[u].x);
            sA[4 * q + 1][i] = static_cast<double>(ra[u].y);
            sA[4 * q + 2][i] = static_cast<double>(ra[u].z);
            sA[4 * q + 3][i] = static_cast<double>(ra[u].w);
        }
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            const int idx = tid + u * kBootThreads, j = idx / QC, q = idx % QC;
            sC[j][4 * q + 0] = static_cast<double>(rc[u].x);
            sC[j][4 * q + 1] = static_cast<double>(rc[u].y);
            sC[j][4 * q + 2] = static_cast<double>(rc[u].z);
            sC[j][4 * q + 3] = static_cast<double>(rc[u].w);
        }
    };

    double acc[TR][TP];
#pragma unroll
    for (int e = 0; e < TR; ++e)
#pragma unroll
        for (int f = 0; f < TP; ++f) acc[e][f] = 0.0;

    load(0);
    for (int c = 0; c < chunks; ++c) {
        stage();
        __syncthreads();
        if (c + 1 < chunks) load((c + 1) * KC);
#pragma unroll 4
        for (int kk = 0; kk < KC; ++kk) {
            double a[TR], b[TP];
#pragma unroll
            for (int e = 0; e < TR; ++e) a[e] = sA[kk][ty * TR + e];
#pragma unroll
            for (int f = 0; f < TP; ++f) b[f] = sC[kk][tx * TP + f];
#pragma unroll
            for (int e = 0; e < TR; ++e)
#pragma unroll
                for (int f = 0; f < TP; ++f) acc[e][f] = fma(a[e], b[f], acc[e][f]);
        }
        __syncthreads();
    }

    // fold: c_i Y_i and c_i Phi_ii over this thread's rows ...
    double q[TP], s[TP];
#pragma unroll
    for (int f = 0; f < TP; ++f) q[f] = s[f] = 0.0;
#pragma unroll
    for (int e = 0; e < TR; ++e) {
        const int k = k0 + ty * TR + e;
        if (k < n_rows) {
            const int i = row_begin + k;
            const double d = static_cast<double>(phi[static_cast<long long>(k) * ld + i]);
            const int *ci = counts + static_cast<size_t>(i) * pstride + p0 + tx * TP;
#pragma unroll
            for (int f = 0; f < TP; ++f) {
                const double cf = static_cast<double>(ci[f]);
                q[f] = fma(cf, acc[e][f], q[f]);
                s[f] = fma(cf, d, s[f]);
            }
        }
    }
    // ... then over the 16 thread rows, in their order
    double(*red)[PT] = sC;
    double *const outs[2] = {part_quad, part_self};
#pragma unroll
    for (int w = 0; w < 2; ++w) {
#pragma unroll
        for (int f = 0; f < TP; ++f) red[ty][tx * TP + f] = w == 0 ? q[f] : s[f];
        __syncthreads();
        if (tid < PT) {
            double t = 0.0;
#pragma unroll
            for (int y = 0; y < 16; ++y) t += red[y][tid];
            outs[w][static_cast<size_t>(blockIdx.x) * pstride + p0 + tid] = t;
        }
        __syncthreads();
    }
}

// out[r] = the partials of resample r over the row blocks, in block order
__global__ __launch_bounds__(kBootThreads) void boot_reduce_kernel(const double *__restrict__ part_quad, const double *__restrict__ part_self, int n_blocks,
                                                                   int pstride, int p, double *__restrict__ quad, double *__restrict__ self)
{
    const int r = blockIdx.x * kBootThreads + threadIdx.x;
    if (r >= p) return;
    double a = 0.0, d = 0.0;
    for (int blk = 0; blk < n_blocks; ++blk) {
        a += part_quad[static_cast<size_t>(blk) * pstride + r];
        d += part_self[static_cast<size_t>(blk) * pstride + r];
    }
    quad[r] = a;
    self[r] = d;
}

struct Layout {
    int npad, pstride, n_blocks;
    size_t counts, part, out;          // bytes of the widest panel's counts table, of one table of its partials, of one output array
};
Layout layout(int n, int n_rows, int n_boot, int panel)
{
    Layout l;
    l.npad = round_up(n, 64);
    l.pstride = round_up(std::min(panel, n_boot), kBootPad);
    l.n_blocks = (n_rows + kBootRows - 1) / kBootRows;
    l.counts = al256(static_cast<size_t>(l.npad) * l.pstride * sizeof(int));
    l.part = al256(static_cast<size_t>(l.n_blocks) * l.pstride * sizeof(double));
    l.out = al256(static_cast<size_t>(n_boot) * sizeof(double));
    return l;
}

}  // namespace

int boot_panel(int n, int n_boot, int hook)
{
    if (hook >= 1) return std::min(hook, kBootMaxPanel);
    // as many resamples as keep the counts table within its budget, in whole tiles: Phi is read once per panel and resample tile
    const size_t fit = kBootCountsBudget / (static_cast<size_t>(round_up(n, 64)) * sizeof(int));
    const int p = static_cast<int>(std::min<size_t>(fit / kBootPad * kBootPad, kBootMaxPanel));
    return std::min(std::max(p, kBootPad), std::max(n_boot, 1));
}

size_t boot_scratch_bytes(int n, int n_rows, int n_boot, int panel)
{
    const Layout l = layout(n, n_rows, n_boot, panel);
    return l.counts + 2 * l.part + 2 * l.out;
}

hipError_t boot_launch(const BootLaunch &L)
{
    const Layout l = layout(L.n, L.n_rows, L.n_boot, L.panel);
    int *counts = reinterpret_cast<int *>(L.scratch);
    double *part_q = reinterpret_cast<double *>(L.scratch + l.counts), *part_s = reinterpret_cast<double *>(L.scratch + l.counts + l.part);
    double *d_quad = reinterpret_cast<double *>(L.scratch + l.counts + 2 * l.part), *d_self = reinterpret_cast<double *>(L.scratch + l.counts + 2 * l.part + l.out);
    hipError_t e = hipSuccess;
    for (int done = 0; done < L.n_boot && e == hipSuccess; done += L.panel) {
        const int p = std::min(L.panel, L.n_boot - done);
        const int ps = round_up(p, kBootPad);                       // this panel's stride (<= l.pstride): a ragged last panel zeroes and walks its own columns only
        e = hipMemsetAsync(counts, 0, static_cast<size_t>(l.npad) * ps * sizeof(int), L.stream);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(boot_counts_kernel, dim3(p), dim3(kBootThreads), 0, L.stream, counts, ps, L.n,
                           static_cast<unsigned long long>(L.seed), static_cast<unsigned>(L.first + done));
        hipLaunchKernelGGL((boot_quad_kernel<kBootTR, kBootTP, kBootKC>), dim3(l.n_blocks, ps / kBootPad), dim3(kBootThreads), 0, L.stream, L.phi, L.ld, L.n,
                           L.row_begin, L.n_rows, counts, ps, part_q, part_s);
        hipLaunchKernelGGL(boot_reduce_kernel, dim3((p + kBootThreads - 1) / kBootThreads), dim3(kBootThreads), 0, L.stream, part_q, part_s, l.n_blocks,
                           ps, p, d_quad + done, d_self + done);
        e = hipGetLastError();
    }
    const size_t bytes = static_cast<size_t>(L.n_boot) * sizeof(double);
    if (e == hipSuccess && L.quad) e = hipMemcpyAsync(L.quad, d_quad, bytes, hipMemcpyDeviceToHost, L.stream);
    if (e == hipSuccess && L.self) e = hipMemcpyAsync(L.self, d_self, bytes, hipMemcpyDeviceToHost, L.stream);
    const hipError_t s = hipStreamSynchronize(L.stream);          // (the caller's arrays outlive what was enqueued)
    return e != hipSuccess ? e : s;
}

}  // namespace genphi
