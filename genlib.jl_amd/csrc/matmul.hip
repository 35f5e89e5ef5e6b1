// matmul.hip -- the product of the resident result with a caller's tall, skinny Float64 panel (genphi_result_matmul) and the
// conjugate-gradient solve over it (genphi_result_solve; its host loop is result_solve.cpp).  include/genphi.h states the
// contract, DESIGN.md 19 the design.  The plan is seen through resident.h only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/genphi.h"
#include "matmul_device.h"
#include "resident.h"
#include "result_solve.h"

using genphi::al256;
using genphi::ResidentView;

namespace {

// Y = Phi X on the resident rows.  A workgroup of 4 waves owns kMmWaves x R consecutive resident rows, a wave R of them, and
// blockIdx.y one tile of KT columns of X.  The wave walks the columns j of its rows in steps of kMmStep = 64 lanes x one quad:
// lane l of step s loads the 16 bytes Phi[row][4 (64 s + l) ..+3] of each of its R rows and multiplies them with the four rows
// of the X tile at the same j, which the workgroup staged in LDS as Float64, column by column (xs[c][j]: the lanes of a wave read
// consecutive 32-byte pieces as two 16-byte reads; by the bank map of ds_read_b128 -- (a / 4) % 64, groups of 16 lanes -- each
// such read is a 2-way conflict at this stride.  A layout without it measured the same times, so the plain one stays).  A chunk of CH columns is staged between two barriers.  Accumulators: R x KT
// doubles per lane, in registers.
//
// The order of the additions of one entry y[r][c] (include/genphi.h) is fixed by n4 = N rounded up to 4 alone: lane l adds the
// products of its columns j, (j / 4) % 64 == l, j < n4, by fma in ascending j from +0; then six rounds of s_l += s_(l ^ t),
// t = 32, 16, 8, 4, 2, 1 (the two partners compute the same sum, so every lane ends with the same bits).  R, KT, CH, the row's
// place in its block and the other columns of the call do not enter.
//
// xd: the tiles of X, tile t at xd + t * KT * n4, column c of a tile n4 doubles long (rows N .. n4 - 1 and the columns beyond k
// are zero: the host packs them).  y: n_rows x k, dense.  A quad at or beyond n4 is neither loaded nor added (ld >= n4, so
// every quad that is loaded lies inside its row).  Rows beyond n_rows in the last block read the last row and store nothing.
constexpr int kMmWaves = 4;                 // waves of a workgroup: each owns R rows
constexpr int kMmStep = 256;                // columns a wave takes per step: 64 lanes x one quad
constexpr int kMmRowsNarrow = 8;            // R of the forms KT = 1, 2, 4: row blocks of 32
constexpr int kMmRowsWide = 4;              // R of the forms KT = 8, 16: row blocks of 16
constexpr int kMmChunkNarrow = 1024;        // CH, columns staged between two barriers: KT <= 4
constexpr int kMmChunkWide8 = 512;          // ... KT = 8
constexpr int kMmChunkWide16 = 256;         // ... KT = 16 (32 KiB of LDS at most in every form)

template <int R, int KT, int CH>
__global__ __launch_bounds__(256) void matmul_kernel(const float *__restrict__ m, long long ld, int n4, int n_rows, int k,
                                                     const double *__restrict__ xd, double *__restrict__ y)
{
    static_assert(CH % kMmStep == 0 && R * KT <= 64, "a step is 256 columns; the fold hands one entry to one lane");
    __shared__ double xs[KT * CH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = ((int)blockIdx.x * kMmWaves + wave) * R;
    const double *xt = xd + (long long)blockIdx.y * KT * n4;
    const float *row[R];
#pragma unroll
    for (int r = 0; r < R; ++r) row[r] = m + (long long)min(row0 + r, n_rows - 1) * ld;
    double acc[R][KT];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < KT; ++c) acc[r][c] = 0.0;

    for (int j0 = 0; j0 < n4; j0 += CH) {
        __syncthreads();                                             // the chunk before has been read
        for (int i = threadIdx.x; i < KT * (CH / 2); i += 256) {
            const int c = i / (CH / 2), jj = (i - c * (CH / 2)) * 2;
            if (j0 + jj < n4)                                        // (n4 % 4 == 0: a pair is inside or outside)
                *reinterpret_cast<double2 *>(&xs[c * CH + jj]) = *reinterpret_cast<const double2 *>(&xt[(long long)c * n4 + j0 + jj]);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < CH / kMmStep; ++s) {
            const int jl = s * kMmStep + lane * 4, jq = j0 + jl;
            if (jq < n4) {
                float4 v[R];
#pragma unroll
                for (int r = 0; r < R; ++r) v[r] = *reinterpret_cast<const float4 *>(row[r] + jq);
#pragma unroll
                for (int c = 0; c < KT; ++c) {
                    const double2 x01 = *reinterpret_cast<const double2 *>(&xs[c * CH + jl]);
                    const double2 x23 = *reinterpret_cast<const double2 *>(&xs[c * CH + jl + 2]);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        double a = acc[r][c];
                        a = fma(static_cast<double>(v[r].x), x01.x, a);
                        a = fma(static_cast<double>(v[r].y), x01.y, a);
                        a = fma(static_cast<double>(v[r].z), x23.x, a);
                        a = fma(static_cast<double>(v[r].w), x23.y, a);
                        acc[r][c] = a;
                    }
                }
            }
        }
    }
    // the fold across the lanes, in the fixed order; then entry (r, c) leaves from lane r * KT + c
    const int c0 = (int)blockIdx.y * KT;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            double a = acc[r][c];
#pragma unroll
            for (int t = 32; t > 0; t >>= 1) a += __shfl_xor(a, t);
            if (lane == r * KT + c && row0 + r < n_rows && c0 + c < k) y[(long long)(row0 + r) * k + c0 + c] = a;
        }
}

struct MmForm { int rows, kt; };            // rows of a workgroup, columns of a tile
inline MmForm matmul_form(int k)
{
    if (k <= 1) return {kMmWaves * kMmRowsNarrow, 1};
    if (k <= 2) return {kMmWaves * kMmRowsNarrow, 2};
    if (k <= 4) return {kMmWaves * kMmRowsNarrow, 4};
    if (k <= 8) return {kMmWaves * kMmRowsWide, 8};
    return {kMmWaves * kMmRowsWide, 16};
}

}  // namespace

int genphi::matmul_panel_columns(int k)
{
    const MmForm f = matmul_form(k);
    return (k + f.kt - 1) / f.kt * f.kt;
}

hipError_t genphi::matmul_on_device(const ResidentView &v, int n4, int k, const double *xd, double *y)
{
    const MmForm f = matmul_form(k);
    const int nr = static_cast<int>(v.n_rows);
    const dim3 grid(static_cast<unsigned>((nr + f.rows - 1) / f.rows), static_cast<unsigned>((k + f.kt - 1) / f.kt));
    const long long ld = static_cast<long long>(v.ld);
    switch (f.kt) {
    case 1: hipLaunchKernelGGL((matmul_kernel<kMmRowsNarrow, 1, kMmChunkNarrow>), grid, dim3(256), 0, v.stream, v.result, ld, n4, nr, k, xd, y); break;
    case 2: hipLaunchKernelGGL((matmul_kernel<kMmRowsNarrow, 2, kMmChunkNarrow>), grid, dim3(256), 0, v.stream, v.result, ld, n4, nr, k, xd, y); break;
    case 4: hipLaunchKernelGGL((matmul_kernel<kMmRowsNarrow, 4, kMmChunkNarrow>), grid, dim3(256), 0, v.stream, v.result, ld, n4, nr, k, xd, y); break;
    case 8: hipLaunchKernelGGL((matmul_kernel<kMmRowsWide, 8, kMmChunkWide8>), grid, dim3(256), 0, v.stream, v.result, ld, n4, nr, k, xd, y); break;
    default: hipLaunchKernelGGL((matmul_kernel<kMmRowsWide, 16, kMmChunkWide16>), grid, dim3(256), 0, v.stream, v.result, ld, n4, nr, k, xd, y); break;
    }
    return hipGetLastError();
}

namespace {

// what both entry points check of k and a panel (x of matmul, b of solve)
int check_panel(const char *name, int32_t k, const char *what, const void *a, int64_t lda)
{
    if (k < 1 || k > GENPHI_MATMUL_MAX_K)
        return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": k = " + std::to_string(k) + " outside [1, " + std::to_string(GENPHI_MATMUL_MAX_K) + "]");
    if (!a) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": " + what + " is NULL");
    if (lda < k) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": the pitch of " + what + " is " + std::to_string(lda) + ", below k = " + std::to_string(k));
    return GENPHI_OK;
}

// not the Float64 result; then *empty for an empty shard (GENPHI_OK), else a resident result with rows
int need_f32_rows(const ResidentView &v, const char *name, bool *empty)
{
    *empty = false;
    if (v.res_f64) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + " works on the Float32 result (gen.phi's matrix)");
    if (v.res_known && v.n_rows == 0) { *empty = true; return GENPHI_OK; }
    if (!v.on_device || !v.result || v.n_rows == 0) return genphi_set_error(GENPHI_ERR_DEVICE, "no resident result: call genphi_compute_device first");
    return GENPHI_OK;
}

}  // namespace

extern "C" {

int genphi_result_matmul(genphi_plan *p, int32_t k, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t *n_rows)
{
    static const char *const name = "genphi_result_matmul";
    if (!p) return genphi_set_error(GENPHI_ERR_ARG, "plan is NULL");
    const ResidentView v = genphi::resident_view(p);
    int rc = check_panel(name, k, "x", x, ldx);
    if (rc) return rc;
    if (ldy < k) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": the pitch of y is " + std::to_string(ldy) + ", below k = " + std::to_string(k));
    bool empty;
    rc = need_f32_rows(v, name, &empty);
    if (rc) return rc;
    if (empty) {
        if (n_rows) *n_rows = 0;
        return GENPHI_OK;
    }
    if (!y) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": y is NULL");
    const int64_t N = v.n_pro, nr = v.n_rows;
    if (v.ld < N || v.ld % 64 != 0) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(name) + ": unexpected row pitch " + std::to_string(v.ld));
    GENPHI_RESIDENT_TRY("hipSetDevice(p->device)", hipSetDevice(v.device));
    // the device copy of X: tiles of kt columns, each column n4 doubles; rows N .. n4 - 1 and the columns k .. kp - 1 are zero,
    // and all of it is written on every call (the scratch block is reused: nothing stale may meet a padding zero of Phi)
    const int n4 = static_cast<int>((N + 3) / 4 * 4);
    const int kp = genphi::matmul_panel_columns(k);
    const size_t x_bytes = al256(static_cast<size_t>(kp) * n4 * sizeof(double)), y_bytes = static_cast<size_t>(nr) * k * sizeof(double);
    char *scratch;
    if (genphi::resident_scratch(p, x_bytes + y_bytes, &scratch) != GENPHI_OK)
        return genphi_set_error(GENPHI_ERR_ALLOC, std::string(name) + ": " + std::to_string(x_bytes + y_bytes) + " bytes of device memory for the panel and the product: " +
                                                      genphi_last_error());
    std::vector<double> packed;
    try {
        packed.assign(static_cast<size_t>(kp) * n4, 0.0);
    } catch (const std::bad_alloc &) {
        return genphi_set_error(GENPHI_ERR_ALLOC, std::string(name) + ": no host memory for the packed panel");
    }
    for (int64_t j = 0; j < N; ++j)
        for (int c = 0; c < k; ++c) packed[static_cast<size_t>(c) * n4 + j] = x[j * ldx + c];
    double *d_x = reinterpret_cast<double *>(scratch), *d_y = reinterpret_cast<double *>(scratch + x_bytes);
    hipError_t e = hipMemcpyAsync(d_x, packed.data(), packed.size() * sizeof(double), hipMemcpyHostToDevice, v.stream);
    if (e == hipSuccess) e = genphi::matmul_on_device(v, n4, k, d_x, d_y);
    if (e == hipSuccess)
        e = hipMemcpy2DAsync(y, static_cast<size_t>(ldy) * sizeof(double), d_y, static_cast<size_t>(k) * sizeof(double), static_cast<size_t>(k) * sizeof(double),
                             static_cast<size_t>(nr), hipMemcpyDeviceToHost, v.stream);
    const hipError_t es = hipStreamSynchronize(v.stream);            // also after an error: the host arrays outlive what was enqueued
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(name) + ": " + hipGetErrorString(e));
    if (n_rows) *n_rows = nr;
    return GENPHI_OK;
}

int genphi_result_solve(genphi_plan *p, int32_t k, const double *b, int64_t ldb, double ridge, double tol, int32_t max_iter, double *z, int64_t ldz,
                        double *residual, int32_t *iterations)
{
    static const char *const name = "genphi_result_solve";
    if (!p) return genphi_set_error(GENPHI_ERR_ARG, "plan is NULL");
    const ResidentView v = genphi::resident_view(p);
    int rc = check_panel(name, k, "b", b, ldb);
    if (rc) return rc;
    if (ldz < k) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": the pitch of z is " + std::to_string(ldz) + ", below k = " + std::to_string(k));
    if (!(ridge >= 0.0) || !std::isfinite(ridge)) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": ridge = " + std::to_string(ridge) + " is negative or not finite");
    if (!(tol >= 0.0)) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": tol = " + std::to_string(tol) + " is negative or NaN");
    if (max_iter < 1) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": max_iter = " + std::to_string(max_iter) + ", need at least 1");
    bool empty;
    rc = need_f32_rows(v, name, &empty);
    if (rc) return rc;
    if (empty || v.n_rows != v.n_pro)
        return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": " + std::to_string(v.n_rows) + " of " + std::to_string(v.n_pro) +
                                                    " rows are resident: a shard cannot solve");
    if (!z) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": z is NULL");
    try {
        return genphi::cg_solve(v.n_pro, k, b, ldb, ridge, tol, max_iter,
                                [p](int32_t kk, const double *x, double *y) { return genphi_result_matmul(p, kk, x, kk, y, kk, nullptr); },
                                z, ldz, residual, iterations);
    } catch (const std::bad_alloc &) {
        return genphi_set_error(GENPHI_ERR_ALLOC, std::string(name) + ": no host memory for the iteration");
    }
}

}  // extern "C"
