// eigen.hip -- the leading eigenpairs of the resident result by Lanczos with full reorthogonalisation, every vector of the iteration
// on the device (genphi_result_eigen).  include/genphi.h states the contract, DESIGN.md 21 the design; the host loop is
// result_eigen.cpp, the product matmul.hip's kernel through matmul_device.h.  The plan is seen through resident.h only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "../../include/genphi.h"
#include "matmul_device.h"
#include "resident.h"
#include "result_eigen.h"

using genphi::al256;
using genphi::ResidentView;

namespace {

// A vector of the iteration is n4 = N rounded up to 4 doubles long, the one-column panel that matmul_kernel reads.  Rows N .. n4 - 1
// of every vector are +0: the whole block is cleared at the start of a call and no kernel below writes a row >= N.
//
// Every sum over the entries of a vector has one order, fixed by n4 alone: thread t of a 256-thread workgroup takes the pairs
// (2 p, 2 p + 1), p = t, t + 256, ..., in ascending p, the even entry first; then six rounds s_l += s_(l ^ t), t = 32 .. 1, inside
// each wave (both partners compute the same sum); then ((s_wave0 + s_wave1) + s_wave2) + s_wave3 through LDS.
constexpr int kEigThreads = 256;                             // threads of a workgroup: four waves
constexpr int kEigStep = 2 * kEigThreads;                    // entries that a workgroup takes per step of a sum: 512
static_assert(kEigThreads == 256 && kEigStep == 512, "block_sum folds four waves; the order of a sum is stated for 256 threads");

__device__ inline double block_sum(double s)
{
    __shared__ double part[kEigThreads / 64];
#pragma unroll
    for (int t = 32; t > 0; t >>= 1) s += __shfl_xor(s, t);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    const double total = ((part[0] + part[1]) + part[2]) + part[3];
    __syncthreads();                                         // (the next sum of this workgroup writes part again)
    return total;
}

// out[b] = a . w, a = basis vector first + b while that is below m, else w itself (w . w).  One workgroup per b.
__global__ __launch_bounds__(kEigThreads) void eig_dots_kernel(const double *__restrict__ basis, const double *__restrict__ w, int n4, int m, int first,
                                                               double *__restrict__ out)
{
    const int i = first + (int)blockIdx.x;
    const double2 *a = reinterpret_cast<const double2 *>(i < m ? basis + (size_t)i * n4 : w);
    const double2 *b = reinterpret_cast<const double2 *>(w);
    double s = 0.0;
    for (int p = threadIdx.x; p < n4 / 2; p += kEigThreads) {
        const double2 x = a[p], y = b[p];
        s = fma(x.x, y.x, s);
        s = fma(x.y, y.y, s);
    }
    s = block_sum(s);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// out[c] = the sum of the entries of column c of x (column c at x + c * n4), in the order above.  One workgroup per column.
__global__ __launch_bounds__(kEigThreads) void eig_sum_kernel(const double *__restrict__ x, int n4, double *__restrict__ out)
{
    const double2 *a = reinterpret_cast<const double2 *>(x + (size_t)blockIdx.x * n4);
    double s = 0.0;
    for (int p = threadIdx.x; p < n4 / 2; p += kEigThreads) {
        const double2 v = a[p];
        s += v.x;
        s += v.y;
    }
    s = block_sum(s);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// dst[c][e] = src[c][e] - sums[c] / n on the rows e < n (dst may be src).  blockIdx.y = c.
__global__ __launch_bounds__(kEigThreads) void eig_centre_kernel(double *dst, const double *src, int n, int n4, const double *__restrict__ sums)
{
    const int e = ((int)blockIdx.x * kEigThreads + (int)threadIdx.x) * 2;
    if (e >= n) return;
    const size_t at = (size_t)blockIdx.y * n4 + e;
    const double mean = sums[blockIdx.y] / (double)n;
    dst[at] = src[at] - mean;
    if (e + 1 < n) dst[at + 1] = src[at + 1] - mean;
}

// w[e] -= sum over i < m of h[i] basis[i][e], ascending i by fma, on the rows e < n.  One thread per pair of rows.
__global__ __launch_bounds__(kEigThreads) void eig_subtract_kernel(const double *__restrict__ basis, double *__restrict__ w, int n, int n4, int m,
                                                                   const double *__restrict__ h)
{
    const int e = ((int)blockIdx.x * kEigThreads + (int)threadIdx.x) * 2;
    if (e >= n) return;
    double2 acc = *reinterpret_cast<const double2 *>(w + e);         // (e + 1 < n4: the pair lies inside the vector)
    for (int i = 0; i < m; ++i) {
        const double2 v = *reinterpret_cast<const double2 *>(basis + (size_t)i * n4 + e);
        const double c = -h[i];
        acc.x = fma(c, v.x, acc.x);
        acc.y = fma(c, v.y, acc.y);
    }
    w[e] = acc.x;
    if (e + 1 < n) w[e + 1] = acc.y;
}

// dst[e] = scale w[e] on the rows e < n
__global__ __launch_bounds__(kEigThreads) void eig_store_kernel(double *__restrict__ dst, const double *__restrict__ w, int n, double scale)
{
    const int e = ((int)blockIdx.x * kEigThreads + (int)threadIdx.x) * 2;
    if (e >= n) return;
    dst[e] = w[e] * scale;
    if (e + 1 < n) dst[e + 1] = w[e + 1] * scale;
}

// u[c][e] = sum over i < m of S[i * k + c] basis[i][e], ascending i by fma from +0, on the rows e < n: the Ritz vectors, written as
// the panel that matmul_kernel reads (column c at u + c * n4).  blockIdx.y = c.
__global__ __launch_bounds__(kEigThreads) void eig_combine_kernel(const double *__restrict__ basis, const double *__restrict__ S, double *__restrict__ u, int n,
                                                                  int n4, int m, int k)
{
    const int e = ((int)blockIdx.x * kEigThreads + (int)threadIdx.x) * 2;
    if (e >= n) return;
    const int c = blockIdx.y;
    double2 acc = make_double2(0.0, 0.0);
    for (int i = 0; i < m; ++i) {
        const double2 v = *reinterpret_cast<const double2 *>(basis + (size_t)i * n4 + e);
        const double s = S[(size_t)i * k + c];
        acc.x = fma(s, v.x, acc.x);
        acc.y = fma(s, v.y, acc.y);
    }
    double *dst = u + (size_t)c * n4 + e;
    dst[0] = acc.x;
    if (e + 1 < n) dst[1] = acc.y;
}

// out[c] = || c(y_c) - theta[c] u_c ||_2 over the rows < n, y the n x k row-major product, c() the subtraction of the column's mean
// when centre is set (else nothing).  One workgroup per column; thread t takes the rows t, t + 256, ... in ascending order.
__global__ __launch_bounds__(kEigThreads) void eig_residual_kernel(const double *__restrict__ y, const double *__restrict__ u, const double *__restrict__ theta,
                                                                   int n, int n4, int k, int centre, double *__restrict__ out)
{
    const int c = blockIdx.x;
    double mean = 0.0;
    if (centre) {
        double s = 0.0;
        for (int r = threadIdx.x; r < n; r += kEigThreads) s += y[(size_t)r * k + c];
        mean = block_sum(s) / (double)n;
    }
    const double th = theta[c];
    double s = 0.0;
    for (int r = threadIdx.x; r < n; r += kEigThreads) {
        const double d = (y[(size_t)r * k + c] - mean) - th * u[(size_t)c * n4 + r];
        s = fma(d, d, s);
    }
    s = block_sum(s);
    if (threadIdx.x == 0) out[c] = sqrt(s);
}

// the device side of genphi::EigenOps: the vectors of one call inside the plan's scratch block
struct EigenDevice {
    ResidentView v;
    int n, n4, steps;
    bool centre;
    double *basis, *w, *xc, *u, *y, *dots, *coef, *sums;
    hipError_t err = hipSuccess;                             // the first HIP error of the call

    unsigned row_blocks() const { return static_cast<unsigned>((n4 / 2 + kEigThreads - 1) / kEigThreads); }
    double *slot(int j) { return j == genphi::kEigenWork ? w : basis + static_cast<size_t>(j) * n4; }
    int done(hipError_t e)
    {
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) return 0;
        if (err == hipSuccess) err = e;
        return GENPHI_ERR_DEVICE;
    }
    int sync(hipError_t e)
    {
        const hipError_t es = hipStreamSynchronize(v.stream);        // also after an error: host arrays outlive what was enqueued
        return done(e == hipSuccess ? es : e);
    }
    // dst = c(src) for `cols` columns
    hipError_t centre_columns(double *dst, const double *src, int cols)
    {
        hipLaunchKernelGGL(eig_sum_kernel, dim3(cols), dim3(kEigThreads), 0, v.stream, src, n4, sums);
        hipLaunchKernelGGL(eig_centre_kernel, dim3(row_blocks(), cols), dim3(kEigThreads), 0, v.stream, dst, src, n, n4, sums);
        return hipGetLastError();
    }

    int set(int32_t j, const double *x) { return sync(hipMemcpyAsync(slot(j), x, static_cast<size_t>(n) * sizeof(double), hipMemcpyHostToDevice, v.stream)); }
    int apply(int32_t j)
    {
        const double *src = slot(j);
        hipError_t e = hipSuccess;
        if (centre) {
            e = centre_columns(xc, src, 1);
            src = xc;
        }
        if (e == hipSuccess) e = genphi::matmul_on_device(v, n4, 1, src, w);   // (one column: the product's n entries are w's rows < n)
        if (e == hipSuccess && centre) e = centre_columns(w, w, 1);
        return done(e);
    }
    int dots_to(int32_t m, int first, int count, double *h)
    {
        hipLaunchKernelGGL(eig_dots_kernel, dim3(count), dim3(kEigThreads), 0, v.stream, basis, w, n4, m, first, dots);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h, dots, static_cast<size_t>(count) * sizeof(double), hipMemcpyDeviceToHost, v.stream);
        return sync(e);
    }
    int project(int32_t m, double *h) { return dots_to(m, 0, m, h); }
    int norm2(double *ww) { return dots_to(0, 0, 1, ww); }
    int subtract(int32_t m, const double *h)
    {
        hipError_t e = hipMemcpyAsync(coef, h, static_cast<size_t>(m) * sizeof(double), hipMemcpyHostToDevice, v.stream);
        if (e == hipSuccess) hipLaunchKernelGGL(eig_subtract_kernel, dim3(row_blocks()), dim3(kEigThreads), 0, v.stream, basis, w, n, n4, m, coef);
        return sync(e);                                              // (h is the caller's again)
    }
    int store(int32_t j, double scale)
    {
        hipLaunchKernelGGL(eig_store_kernel, dim3(row_blocks()), dim3(kEigThreads), 0, v.stream, slot(j), w, n, scale);
        return done(hipSuccess);
    }
    int combine(int32_t m, int32_t kk, const double *S)
    {
        hipError_t e = hipMemcpyAsync(coef, S, static_cast<size_t>(m) * kk * sizeof(double), hipMemcpyHostToDevice, v.stream);
        if (e == hipSuccess) hipLaunchKernelGGL(eig_combine_kernel, dim3(row_blocks(), kk), dim3(kEigThreads), 0, v.stream, basis, coef, u, n, n4, m, kk);
        if (e == hipSuccess && centre) e = centre_columns(u, u, kk);  // Op reads c(u): the vectors that leave are these
        return sync(e);
    }
    int residuals(int32_t kk, const double *theta, double *out)
    {
        hipError_t e = hipMemcpyAsync(coef, theta, static_cast<size_t>(kk) * sizeof(double), hipMemcpyHostToDevice, v.stream);
        if (e == hipSuccess) e = genphi::matmul_on_device(v, n4, kk, u, y);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(eig_residual_kernel, dim3(kk), dim3(kEigThreads), 0, v.stream, y, u, coef, n, n4, kk, centre ? 1 : 0, dots);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(out, dots, static_cast<size_t>(kk) * sizeof(double), hipMemcpyDeviceToHost, v.stream);
        return sync(e);
    }
    int download(int32_t kk, double *vectors, int64_t ldv)
    {
        std::vector<double> col(static_cast<size_t>(kk) * n4);
        const int rc = sync(hipMemcpyAsync(col.data(), u, col.size() * sizeof(double), hipMemcpyDeviceToHost, v.stream));
        if (rc) return rc;
        for (int64_t e = 0; e < n; ++e)
            for (int32_t c = 0; c < kk; ++c) vectors[e * ldv + c] = col[static_cast<size_t>(c) * n4 + e];
        return 0;
    }
};

}  // namespace

extern "C" int genphi_result_eigen(genphi_plan *p, int32_t k, int32_t center, double tol, int32_t max_iter, uint64_t seed, double *values, double *vectors,
                                   int64_t ldv, double *residual, int32_t *converged, int32_t *products)
{
    const std::string name = "genphi_result_eigen";
    if (!p) return genphi_set_error(GENPHI_ERR_ARG, "plan is NULL");
    const ResidentView v = genphi::resident_view(p);
    const int64_t N = v.n_pro;
    if (k < 1 || k > GENPHI_EIGEN_MAX_K || k > N)
        return genphi_set_error(GENPHI_ERR_ARG, name + ": k = " + std::to_string(k) + " outside [1, min(" + std::to_string(GENPHI_EIGEN_MAX_K) + ", N = " + std::to_string(N) + ")]");
    if (!(tol >= 0.0)) return genphi_set_error(GENPHI_ERR_ARG, name + ": tol = " + std::to_string(tol) + " is negative or NaN");
    if (max_iter < k || max_iter > genphi::kEigenMaxIter)
        return genphi_set_error(GENPHI_ERR_ARG, name + ": max_iter = " + std::to_string(max_iter) + " outside [k = " + std::to_string(k) + ", " + std::to_string(genphi::kEigenMaxIter) + "]");
    if (ldv < k) return genphi_set_error(GENPHI_ERR_ARG, name + ": the pitch of vectors is " + std::to_string(ldv) + ", below k = " + std::to_string(k));
    if (v.res_f64) return genphi_set_error(GENPHI_ERR_ARG, name + " works on the Float32 result (gen.phi's matrix)");
    const bool empty = v.res_known && v.n_rows == 0;
    if (!empty && (!v.on_device || !v.result || v.n_rows == 0)) return genphi_set_error(GENPHI_ERR_DEVICE, "no resident result: call genphi_compute_device first");
    if (empty || v.n_rows != N)
        return genphi_set_error(GENPHI_ERR_ARG, name + ": " + std::to_string(v.n_rows) + " of " + std::to_string(N) + " rows are resident: a shard cannot iterate");
    if (!values || !vectors) return genphi_set_error(GENPHI_ERR_ARG, name + (values ? ": vectors is NULL" : ": values is NULL"));
    if (v.ld < N || v.ld % 64 != 0) return genphi_set_error(GENPHI_ERR_DEVICE, name + ": unexpected row pitch " + std::to_string(v.ld));
    GENPHI_RESIDENT_TRY("hipSetDevice(p->device)", hipSetDevice(v.device));

    EigenDevice d{};
    d.v = v;
    d.n = static_cast<int>(N);
    d.n4 = static_cast<int>((N + 3) / 4 * 4);
    d.steps = static_cast<int>(std::min<int64_t>(max_iter, N));
    d.centre = center != 0;
    // one block, sized up front (growing it would lose the basis): the basis, w, c(v), the Ritz panel, its product, and the scalars
    const size_t vec = static_cast<size_t>(d.n4) * sizeof(double);
    const size_t basis_b = al256((static_cast<size_t>(d.steps) + 1) * vec), vec_b = al256(vec), u_b = al256(static_cast<size_t>(genphi::matmul_panel_columns(k)) * vec);
    const size_t y_b = al256(static_cast<size_t>(N) * k * sizeof(double)), dots_b = al256((static_cast<size_t>(d.steps) + 2 + k) * sizeof(double));
    const size_t coef_b = al256((static_cast<size_t>(d.steps) * k + d.steps + 1 + k) * sizeof(double)), sums_b = al256(GENPHI_EIGEN_MAX_K * sizeof(double));
    const size_t bytes = basis_b + 2 * vec_b + u_b + y_b + dots_b + coef_b + sums_b;
    char *scratch;
    if (genphi::resident_scratch(p, bytes, &scratch) != GENPHI_OK)
        return genphi_set_error(GENPHI_ERR_ALLOC, name + ": " + std::to_string(bytes) + " bytes of device memory for the basis of " + std::to_string(d.steps) +
                                                      " steps, the Ritz panel and its product: " + genphi_last_error());
    char *at = scratch;
    auto take = [&at](size_t b) { double *q = reinterpret_cast<double *>(at); at += b; return q; };
    d.basis = take(basis_b);
    d.w = take(vec_b);
    d.xc = take(vec_b);
    d.u = take(u_b);
    d.y = take(y_b);
    d.dots = take(dots_b);
    d.coef = take(coef_b);
    d.sums = take(sums_b);
    // every byte +0: the padding rows of all vectors and the padding columns of the panel, whatever an earlier call left here
    GENPHI_RESIDENT_TRY("hipMemsetAsync(scratch)", hipMemsetAsync(scratch, 0, bytes, v.stream));

    genphi::EigenOps ops;
    ops.set = [&d](int32_t j, const double *x) { return d.set(j, x); };
    ops.apply = [&d](int32_t j) { return d.apply(j); };
    ops.project = [&d](int32_t m, double *h) { return d.project(m, h); };
    ops.subtract = [&d](int32_t m, const double *h) { return d.subtract(m, h); };
    ops.norm2 = [&d](double *ww) { return d.norm2(ww); };
    ops.store = [&d](int32_t j, double scale) { return d.store(j, scale); };
    ops.combine = [&d](int32_t m, int32_t kk, const double *S) { return d.combine(m, kk, S); };
    ops.residuals = [&d](int32_t kk, const double *theta, double *out) { return d.residuals(kk, theta, out); };
    ops.download = [&d](int32_t kk, double *vv, int64_t ld) { return d.download(kk, vv, ld); };
    int rc;
    try {
        rc = genphi::lanczos_top(N, k, d.centre, tol, max_iter, seed, ops, values, vectors, ldv, residual, converged, products);
    } catch (const std::bad_alloc &) {
        (void)hipStreamSynchronize(v.stream);
        return genphi_set_error(GENPHI_ERR_ALLOC, name + ": no host memory for the iteration");
    }
    if (rc) {
        (void)hipStreamSynchronize(v.stream);
        return genphi_set_error(rc, name + ": " + (d.err != hipSuccess ? hipGetErrorString(d.err) : "the iteration failed"));
    }
    return GENPHI_OK;
}
