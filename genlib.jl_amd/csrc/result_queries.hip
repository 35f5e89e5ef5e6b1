// result_queries.hip -- the queries of the finished resident result (include/genphi.h, genphi_result_*): kernels that read the
// proband x proband matrix where the sweep left it, and their entry points.  They see the plan through resident.h only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/genphi.h"
#include "bootstrap.h"
#include "group_tables.h"
#include "over_device.h"
#include "resident.h"

using genphi::al256;
using genphi::ResidentView;
using genphi::kGsMaxGroups;
using genphi::kGsTile;
using genphi::kOverTile;
using genphi::over_hits;
using genphi::kNearBufMin;      // (tuning.h, with the clamp that tuning_from applies)

namespace {

// point lookups in the resident result (genphi_result_entries): out[k] = m[off[k]] widened
__global__ void gather_entries_kernel(const float *__restrict__ m, const long long *__restrict__ off, long long n,
                                      double *__restrict__ out)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = static_cast<double>(m[off[k]]);
}

__global__ void gather_entries64_kernel(const double *__restrict__ m, const long long *__restrict__ off, long long n,
                                        double *__restrict__ out)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = m[off[k]];
}

// phiMean support: Float64 sum of each resident row and its diagonal entry (row r0 + k holds
// proband r0 + k).  One workgroup per row, fixed summation order => reproducible.
__global__ void row_sums_kernel(const float *m, long long ld, int n, int row_begin, double *row_sum, double *diag)
{
    __shared__ double part[256];
    const int k = blockIdx.x;
    const float *row = m + (long long)k * ld;
    double acc = 0.0;
    for (int j = threadIdx.x * 4; j < n; j += blockDim.x * 4) {       // ld is a multiple of 64 and columns >= n are zero
        const float4 v = *reinterpret_cast<const float4 *>(row + j);
        acc += (static_cast<double>(v.x) + static_cast<double>(v.y)) + (static_cast<double>(v.z) + static_cast<double>(v.w));
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s2 = blockDim.x >> 1; s2 > 0; s2 >>= 1) {
        if ((int)threadIdx.x < s2) part[threadIdx.x] += part[threadIdx.x + s2];
        __syncthreads();
    }
    if (threadIdx.x == 0) { row_sum[k] = part[0]; diag[k] = static_cast<double>(row[row_begin + k]); }
}

// gen.phiOver support (genphi_result_over): the pairs (i, j), i < j < n, of the resident rows with
// (double)Phi[i][j] >= t, listed by row, then by column.  One workgroup per resident row walks the columns right of the diagonal
// in place, a tile of kOverTile columns at a time, one quad per thread.  The first quad of a row is loaded whole (16-byte
// aligned; ld is a multiple of 64) and its columns <= i are masked out; so are the padding columns >= n, which a threshold
// <= 0 would select.  over_count_kernel leaves one count per row; the host turns the counts into offsets; over_write_kernel
// repeats the walk and gives every hit its place by an exclusive scan over the tile (three ballots over the bits of the
// per-thread counts 0..4, the four wave totals through LDS): no atomics, so the order is row, column whatever the launch
// geometry.  Both kernels test the same bits with the same expression, so the second pass finds what the first counted.
// The tile and the edge test (over_hits) are in over_device.h: the cluster queries (clusters.hip) test the same bits.

__global__ __launch_bounds__(256) void over_count_kernel(const float *__restrict__ m, long long ld, int n, int row_begin, double t,
                                                         long long *__restrict__ row_count)
{
    __shared__ int part[4];
    const int k = blockIdx.x, i = row_begin + k;
    const float *row = m + (long long)k * ld;
    int cnt = 0;
#pragma unroll 4
    for (int jq = ((i + 1) & ~3) + (int)threadIdx.x * 4; jq < n; jq += kOverTile)
        cnt += __popc(over_hits(*reinterpret_cast<const float4 *>(row + jq), jq, i, n, t));
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_down(cnt, s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) row_count[k] = (long long)part[0] + part[1] + part[2] + part[3];
}

// row_off: nr + 1 offsets (exclusive scan of the counts); total = row_off[nr], the entries of each output array
__global__ __launch_bounds__(256) void over_write_kernel(const float *__restrict__ m, long long ld, int n, int row_begin, double t,
                                                         const long long *__restrict__ row_off, long long total,
                                                         int *__restrict__ out_row, int *__restrict__ out_col, float *__restrict__ out_val)
{
    __shared__ int wtot[2][4];
    const int k = blockIdx.x, i = row_begin + k;
    long long base = row_off[k];
    if (row_off[k + 1] == base) return;                  // (the whole workgroup) a row without a hit is not read again
    const float *row = m + (long long)k * ld;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    int jq = ((i + 1) & ~3) + (int)threadIdx.x * 4;
    float4 v = zero;
    if (jq < n) v = *reinterpret_cast<const float4 *>(row + jq);
    for (int j0 = (i + 1) & ~3, par = 0; j0 < n; j0 += kOverTile, jq += kOverTile, par ^= 1) {
        float4 nxt = zero;
        if (jq + kOverTile < n) nxt = *reinterpret_cast<const float4 *>(row + jq + kOverTile);      // in flight across the scan
        const unsigned hits = over_hits(v, jq, i, n, t);              // (jq >= n: every column masked)
        const int c = __popc(hits);
        const unsigned long long b0 = __ballot(c & 1), b1 = __ballot(c & 2), b2 = __ballot(c & 4);
        const unsigned long long below = (1ull << lane) - 1ull;
        const int before = __popcll(b0 & below) + 2 * __popcll(b1 & below) + 4 * __popcll(b2 & below);
        if (lane == 0) wtot[par][wave] = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
        __syncthreads();                                 // one barrier per tile: tile T + 2 reuses wtot[par] only after every wave passed T + 1's
        int wbase = 0, tile_total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int x = wtot[par][w];
            if (w < wave) wbase += x;
            tile_total += x;
        }
        long long pos = base + wbase + before;
        if (pos + c <= total) {                          // always true while counts and result belong together; never write past the lists
            if (hits & 1u) { out_row[pos] = i; out_col[pos] = jq; out_val[pos] = v.x; ++pos; }
            if (hits & 2u) { out_row[pos] = i; out_col[pos] = jq + 1; out_val[pos] = v.y; ++pos; }
            if (hits & 4u) { out_row[pos] = i; out_col[pos] = jq + 2; out_val[pos] = v.z; ++pos; }
            if (hits & 8u) { out_row[pos] = i; out_col[pos] = jq + 3; out_val[pos] = v.w; ++pos; }
        }
        base += tile_total;
        v = nxt;
    }
}

// gen.phiNearest support (genphi_result_nearest): per resident row i its k best candidates -- the columns j < n,
// j != i, by larger Phi[i][j] first and smaller j first among equal values.  Every entry of a sweep is >= +0, so the 64-bit key
// (value bits << 32) | (0xFFFFFFFF - j) orders the candidates exactly so; no two keys of a row are equal and every key is > 0.
// One workgroup per resident row walks the WHOLE row once, in place, a tile of kNearTile columns at a time (kNearQuads 16-byte
// loads per thread, the next tile's in flight).  It keeps a buffer of `cap` keys in LDS and a threshold tau (0 at first): the keys
// > tau of a tile are appended at places given by an exclusive scan over the tile (ballots over the bits of the per-thread counts,
// the four wave totals through LDS, as over_write_kernel does: no atomics).  When a tile's keys do not all fit, the buffer is
// filled to the brim, sorted (bitonic, descending), cut to its k largest, tau becomes the k-th largest -- a key <= tau can no
// longer be among the k nearest -- and the rest of the tile is tested against the new tau and appended, as often as it takes.
// At the end the survivors are sorted and the first k leave as (column, value).  What is selected and in which order is fixed by
// the keys alone: cap, the tile and the order of appends change how often the buffer is cut, never the output.
constexpr int kNearQuads = 4;                         // 16-byte loads per thread and tile
constexpr int kNearTile = 256 * 4 * kNearQuads;       // columns of a tile

// descending bitonic sort of buf[0, P), P a power of two, by the 256 threads of the workgroup; ends with a barrier
__device__ __forceinline__ void near_sort_desc(unsigned long long *buf, int P)
{
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += 256) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const unsigned long long a = buf[lo], b = buf[hi];
                if ((lo & k2) == 0 ? a < b : a > b) { buf[lo] = b; buf[hi] = a; }
            }
            __syncthreads();
        }
}

__device__ __forceinline__ unsigned long long near_key(float v, int j)
{
    return (static_cast<unsigned long long>(__float_as_uint(v)) << 32) | (0xFFFFFFFFu - static_cast<unsigned>(j));
}

// bit 4 q + e = column jq[q] + e is a candidate with a key > tau
__device__ __forceinline__ unsigned near_hits(const float4 (&v)[kNearQuads], int jq0, int i, int n, unsigned long long tau)
{
    unsigned hits = 0;
#pragma unroll
    for (int q = 0; q < kNearQuads; ++q) {
        const int jq = jq0 + q * 1024;
        const int hi = min(max(n - jq, 0), 4), d = i - jq;
        unsigned valid = ~(0xFu << hi) & 0xFu;                       // left of the padding
        if (d >= 0 && d < 4) valid &= ~(1u << d);                    // not the diagonal
        const unsigned h = (near_key(v[q].x, jq) > tau ? 1u : 0u) | (near_key(v[q].y, jq + 1) > tau ? 2u : 0u) |
                           (near_key(v[q].z, jq + 2) > tau ? 4u : 0u) | (near_key(v[q].w, jq + 3) > tau ? 8u : 0u);
        hits |= (h & valid) << (4 * q);
    }
    return hits;
}

// out_col / out_val: n_rows x k, row-major (either may be null); cap: keys of the dynamic LDS buffer, a power of two in
// [kNearBufMin, kNearBufMax]; 1 <= k <= min(n - 1, 64)
__global__ __launch_bounds__(256) void nearest_kernel(const float *__restrict__ m, long long ld, int n, int row_begin, int k, int cap,
                                                      int *__restrict__ out_col, float *__restrict__ out_val)
{
    extern __shared__ unsigned long long near_buf[];                 // cap keys
    __shared__ int wtot[2][4];
    const int r = blockIdx.x, i = row_begin + r;
    const float *row = m + (long long)r * ld;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned long long tau = 0;
    int cnt = 0, par = 0;                                            // keys in the buffer (the same in every thread)
    float4 v[kNearQuads], nxt[kNearQuads];
    int jq0 = (int)threadIdx.x * 4;
#pragma unroll
    for (int q = 0; q < kNearQuads; ++q) {
        v[q] = zero;
        if (jq0 + q * 1024 < n) v[q] = *reinterpret_cast<const float4 *>(row + jq0 + q * 1024);
    }
    for (int j0 = 0; j0 < n; j0 += kNearTile, jq0 += kNearTile) {
#pragma unroll
        for (int q = 0; q < kNearQuads; ++q) {
            nxt[q] = zero;
            if (jq0 + kNearTile + q * 1024 < n) nxt[q] = *reinterpret_cast<const float4 *>(row + jq0 + kNearTile + q * 1024);
        }
        unsigned pending = near_hits(v, jq0, i, n, tau);             // (a quad at or beyond n: every column masked)
        for (;;) {
            const int c = __popc(pending);                           // 0 .. 16
            const unsigned long long b0 = __ballot(c & 1), b1 = __ballot(c & 2), b2 = __ballot(c & 4), b3 = __ballot(c & 8),
                                     b4 = __ballot(c & 16);
            const int before = __popcll(b0 & below) + 2 * __popcll(b1 & below) + 4 * __popcll(b2 & below) + 8 * __popcll(b3 & below) +
                               16 * __popcll(b4 & below);
            if (lane == 0) wtot[par][wave] = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2) + 8 * __popcll(b3) + 16 * __popcll(b4);
            __syncthreads();                                         // one barrier per round: round R + 2 reuses wtot[par] only after every wave passed R + 1's
            int wbase = 0, total = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int x = wtot[par][w];
                if (w < wave) wbase += x;
                total += x;
            }
            par ^= 1;
            if (total == 0) break;                                   // (the whole workgroup: total is the same in every thread)
            int pos = cnt + wbase + before;
#pragma unroll
            for (int q = 0; q < kNearQuads; ++q) {
                const int jq = jq0 + q * 1024;
                const float e4[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned bit = 1u << (4 * q + e);
                    if (pending & bit) {
                        if (pos < cap) { near_buf[pos] = near_key(e4[e], jq + e); pending &= ~bit; }   // never past the buffer
                        ++pos;
                    }
                }
            }
            if (cnt + total <= cap) { cnt += total; break; }
            // the buffer is full (cap keys) and some of the tile's keys wait: keep the k largest, raise tau, test the rest again
            __syncthreads();
            near_sort_desc(near_buf, cap);
            tau = near_buf[k - 1];
            cnt = k;
            pending &= near_hits(v, jq0, i, n, tau);
            // (the next round's appends go to places >= k; its barrier comes before any thread reads the buffer again)
        }
#pragma unroll
        for (int q = 0; q < kNearQuads; ++q) v[q] = nxt[q];
    }
    // cnt >= k: a key is dropped only when k larger ones are known
    int P = kNearBufMin;
    while (P < cnt) P <<= 1;                                         // <= cap
    for (int t = cnt + (int)threadIdx.x; t < P; t += 256) near_buf[t] = 0;      // below every key
    __syncthreads();
    near_sort_desc(near_buf, P);
    if ((int)threadIdx.x < k) {
        const unsigned long long key = near_buf[threadIdx.x];
        const long long o = (long long)r * k + threadIdx.x;
        if (out_col) out_col[o] = static_cast<int>(0xFFFFFFFFu - static_cast<unsigned>(key));
        if (out_val) out_val[o] = __uint_as_float(static_cast<unsigned>(key >> 32));
    }
}

// Group sums of the resident result (genphi_result_group_sums): T = Phi B summed over blocks of rows.
// A workgroup owns a block of at most kGsBlockRows resident rows of ONE group and a slab of column tiles (kGsTile columns
// each).  Per tile a thread keeps the Float64 column sums of its quad over the block's rows, read in place with 16-byte
// loads, row after row: the labels cost nothing there.  Once per tile (not per row) the 1,024 column sums go through LDS and
// are folded by two host-built tables that are the same for every row: list A cuts the tile's labelled columns into pieces of
// at most kGsPiece columns of one group, list B names the pieces of each group present in the tile (a group appears in it
// once).  One thread owns a piece, then a group: no atomics, fixed summation order => reproducible.  GATHER = false (form
// 0): every group is one run of columns and a piece is a stretch of the tile; GATHER = true (form 1): labels in any order, a
// piece is a stretch of `perm`, the tile's columns sorted by group.  The column sums sit at i + i / 16 so that the piece
// owners, 16 doubles apart, read distinct banks.  LDS and registers are the same for every n_groups: bins has the cap's size.

template <bool GATHER>
__global__ void __launch_bounds__(256)
group_tiles_kernel(const float *__restrict__ m, long long ld, int row_begin, const int *__restrict__ rowlist,
                   const int2 *__restrict__ blocks /* first entry of rowlist, rows */, const int2 *__restrict__ tile_lists /* first A entry, first B entry; n_tiles + 1 */,
                   const int *__restrict__ list_a /* first column | columns << 16 */, const int2 *__restrict__ list_b /* first piece | pieces << 16, group */,
                   const unsigned short *__restrict__ perm, int n_tiles, int tiles_per_slab, int n_slabs, int n_groups,
                   double *__restrict__ part /* [block x slab][n_groups + 1] */)
{
    __shared__ double bins[kGsMaxGroups + 1];
    __shared__ double cs[kGsTile + kGsTile / 16];
    __shared__ double pa[kGsTile];
    const int tid = threadIdx.x;
    const int blk = blockIdx.x / n_slabs, slab = blockIdx.x - blk * n_slabs;
    const int2 b = blocks[blk];
    const int *rows = rowlist + b.x;
    const int nb = b.y;
    for (int g = tid; g <= n_groups; g += 256) bins[g] = 0.0;
    const int t_end = min(n_tiles, (slab + 1) * tiles_per_slab);
    for (int t = slab * tiles_per_slab; t < t_end; ++t) {
        const long long j = (long long)t * kGsTile + tid * 4;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        if (j < ld) {                                                 // ld is a multiple of 64 and columns >= n are zero
            const float *col = m + j;
            int r = 0;
            for (; r + 8 <= nb; r += 8) {
                float4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4 *>(col + (long long)rows[r + u] * ld);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    a0 += static_cast<double>(v[u].x); a1 += static_cast<double>(v[u].y);
                    a2 += static_cast<double>(v[u].z); a3 += static_cast<double>(v[u].w);
                }
            }
            for (; r < nb; ++r) {
                const float4 v = *reinterpret_cast<const float4 *>(col + (long long)rows[r] * ld);
                a0 += static_cast<double>(v.x); a1 += static_cast<double>(v.y);
                a2 += static_cast<double>(v.z); a3 += static_cast<double>(v.w);
            }
        }
        const int c = tid * 4 + (tid >> 2);
        cs[c] = a0; cs[c + 1] = a1; cs[c + 2] = a2; cs[c + 3] = a3;
        __syncthreads();
        const int2 l0 = tile_lists[t], l1 = tile_lists[t + 1];
        const int n_a = l1.x - l0.x, n_b = l1.y - l0.y;
        for (int i = tid; i < n_a; i += 256) {
            const int w = list_a[l0.x + i], first = w & 0xffff, len = w >> 16;
            double s = 0.0;
            for (int k = 0; k < len; ++k) {
                const int e = GATHER ? perm[(long long)t * kGsTile + first + k] : first + k;
                s += cs[e + (e >> 4)];
            }
            pa[i] = s;
        }
        __syncthreads();
        for (int i = tid; i < n_b; i += 256) {
            const int2 w = list_b[l0.y + i];
            const int first = w.x & 0xffff, len = w.x >> 16;
            double s = 0.0;
            for (int k = 0; k < len; ++k) s += pa[first + k];
            bins[w.y] += s;                                           // the only owner of group w.y in this tile
        }
        // (the next tile writes cs before its barrier and pa after it: nothing of this tile is still being read by then)
    }
    if (slab == 0) {                                                  // diagonal entries of the block's rows, in row order
        __syncthreads();
        if (tid < nb) cs[tid] = static_cast<double>(m[(long long)rows[tid] * ld + row_begin + rows[tid]]);
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int k = 0; k < nb; ++k) s += cs[k];
            bins[n_groups] = s;
        }
    }
    __syncthreads();
    double *out = part + (long long)blockIdx.x * (n_groups + 1);
    for (int g = tid; g <= n_groups; g += 256) out[g] = bins[g];
}

// S = A^T T in fixed order: out[k][c] = in[beg[k]][c] + ... + in[beg[k + 1] - 1][c], one thread per entry, applied level by
// level (at most kGsFan rows of one group per output row) until every group has one row.
__global__ void group_rows_reduce_kernel(const double *__restrict__ in, double *__restrict__ out, const int *__restrict__ beg, int width)
{
    const int c = blockIdx.y * blockDim.x + threadIdx.x, k = blockIdx.x;
    if (c >= width) return;
    double s = 0.0;
    for (int r = beg[k]; r < beg[k + 1]; ++r) s += in[(long long)r * width + c];
    out[(long long)k * width + c] = s;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// host side: what the entry points share
// ---------------------------------------------------------------------------------------------
#define SET_DEVICE(v) GENPHI_RESIDENT_TRY("hipSetDevice(p->device)", hipSetDevice((v).device))

// The preconditions of a query of the Float32 result, after its own argument checks: not the Float64 result (`why`: what the
// message says the Float32 one is), then an empty shard -- *empty, GENPHI_OK: it adds nothing -- else a resident result with rows.
static int need_f32_result(const ResidentView &v, const char *name, const char *why, bool *empty)
{
    *empty = false;
    if (v.res_f64) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + " works on the Float32 result (" + why + ")");
    if (v.res_known && v.n_rows == 0) { *empty = true; return GENPHI_OK; }
    if (!v.on_device || !v.result || v.n_rows == 0) return genphi_set_error(GENPHI_ERR_DEVICE, "no resident result: call genphi_compute_device first");
    return GENPHI_OK;
}
static const char *const kPhiMatrix = "gen.phi's matrix", *const kPhiMeanInput = "phiMean's input type, src/compute.jl:454";

// the plan's scratch block grown to `bytes`; a failure names the query and what the memory is for
static int scratch_for(genphi_plan *p, size_t bytes, const char *name, const std::string &what, char **scratch)
{
    if (genphi::resident_scratch(p, bytes, scratch) == GENPHI_OK) return GENPHI_OK;
    return genphi_set_error(GENPHI_ERR_ALLOC, std::string(name) + ": " + std::to_string(bytes) + " bytes of device memory for " + what + ": " + genphi_last_error());
}

// The end of a query: after what was enqueued with status e, one copy per array the caller asked for (dst may be NULL), a
// synchronise -- also after an error: the host arrays outlive what was enqueued -- and the first error under the query's name.
struct CopyBack { void *dst; const void *src; size_t bytes; };
static int copy_back(const ResidentView &v, hipError_t e, std::initializer_list<CopyBack> copies, const char *name)
{
    for (const CopyBack &c : copies)
        if (e == hipSuccess && c.dst) e = hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, v.stream);
    const hipError_t es = hipStreamSynchronize(v.stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(name) + ": " + hipGetErrorString(e));
    return GENPHI_OK;
}

extern "C" {

int genphi_result_device(const genphi_plan *p, const float **d_ptr, int64_t *ld, int64_t *row_begin, int64_t *n_rows)
{
    if (!p) return genphi_set_error(GENPHI_ERR_ARG, "plan is NULL");
    const ResidentView v = genphi::resident_view(p);
    if (v.res_f64) return genphi_set_error(GENPHI_ERR_ARG, "the resident result is Float64 (GENPHI_FLAG_STORAGE_F64): use genphi_result_to_host_f64 / genphi_result_entries");
    if (d_ptr) *d_ptr = v.result;
    if (ld) *ld = v.ld;
    if (row_begin) *row_begin = v.row_begin;
    if (n_rows) *n_rows = v.n_rows;
    return GENPHI_OK;
}

int genphi_result_sums(genphi_plan *p, double *sum_all, double *sum_diag, int64_t *n_rows_out)
{
    if (!p) return genphi_set_error(GENPHI_ERR_ARG, "plan is NULL");
    const ResidentView v = genphi::resident_view(p);
    if (sum_all) *sum_all = 0.0;
    if (sum_diag) *sum_diag = 0.0;
    if (n_rows_out) *n_rows_out = v.n_rows;
    if (v.n_rows == 0 || v.n_pro == 0) return GENPHI_OK;
    bool empty;
    int rc = need_f32_result(v, "genphi_result_sums", kPhiMeanInput, &empty);
    if (rc) return rc;
    SET_DEVICE(v);
    const int64_t nr = v.n_rows;
    char *scratch;
    rc = genphi::resident_scratch(p, 2 * nr * sizeof(double), &scratch);
    if (rc) return rc;
    double *d = reinterpret_cast<double *>(scratch);
    hipLaunchKernelGGL(row_sums_kernel, dim3(static_cast<unsigned>(nr)), dim3(256), 0, v.stream, v.result,
                       static_cast<long long>(v.ld), static_cast<int>(v.n_pro), static_cast<int>(v.row_begin),
                       d, d + nr);
    std::vector<double> h(2 * nr);
    rc = copy_back(v, hipGetLastError(), {{h.data(), d, 2 * nr * sizeof(double)}}, "genphi_result_sums");
    if (rc) return rc;
    double sa = 0.0, sd = 0.0;                      // fixed order: reproducible
    for (int64_t k = 0; k < nr; ++k) { sa += h[k]; sd += h[nr + k]; }
    if (sum_all) *sum_all = sa;
    if (sum_diag) *sum_diag = sd;
    return GENPHI_OK;
}

// gen.phiOver: counting pass -> offsets on the host (in row order, as genphi_result_sums adds its row sums) ->
// writing pass into three lists in the plan's scratch block -> one copy per array the caller asked for.
int genphi_result_over(genphi_plan *p, double threshold, int64_t cap, int32_t *rows, int32_t *cols, float *values, int64_t *n_pairs)
{
    if (!p) return genphi_set_error(GENPHI_ERR_ARG, "plan is NULL");
    const ResidentView v = genphi::resident_view(p);
    if (n_pairs) *n_pairs = 0;
    if (threshold != threshold) return genphi_set_error(GENPHI_ERR_ARG, "genphi_result_over: the threshold is NaN");
    if (cap < 0) return genphi_set_error(GENPHI_ERR_ARG, "genphi_result_over: cap = " + std::to_string(cap) + " is negative");
    const int64_t N = v.n_pro, nr = v.n_rows;
    if (N < 2) return GENPHI_OK;
    bool empty;
    int rc = need_f32_result(v, "genphi_result_over", kPhiMatrix, &empty);
    if (rc || empty) return rc;
    SET_DEVICE(v);
    const size_t off_bytes = al256(static_cast<size_t>(nr + 1) * sizeof(long long));
    const long long ld = static_cast<long long>(v.ld);
    const int n = static_cast<int>(N), r0 = static_cast<int>(v.row_begin);
    genphi::OverCache &oc = genphi::resident_over_cache(p);
    const bool same = oc.valid && static_cast<int64_t>(oc.off.size()) == nr + 1 && std::memcmp(&oc.threshold, &threshold, sizeof(double)) == 0;
    char *scratch;
    if (!same) {
        oc.valid = false;
        rc = scratch_for(p, off_bytes, "genphi_result_over", "the per-row counts", &scratch);
        if (rc) return rc;
        long long *d_cnt = reinterpret_cast<long long *>(scratch);
        hipLaunchKernelGGL(over_count_kernel, dim3(static_cast<unsigned>(nr)), dim3(256), 0, v.stream, v.result, ld, n, r0, threshold, d_cnt);
        std::vector<long long> h(static_cast<size_t>(nr));
        rc = copy_back(v, hipGetLastError(), {{h.data(), d_cnt, static_cast<size_t>(nr) * sizeof(long long)}}, "genphi_result_over (counting pass)");
        if (rc) return rc;
        oc.off.assign(static_cast<size_t>(nr) + 1, 0);
        for (int64_t k = 0; k < nr; ++k) oc.off[k + 1] = oc.off[k] + h[k];
        oc.threshold = threshold;
        oc.valid = true;
    }
    const int64_t total = oc.off[nr];
    if (n_pairs) *n_pairs = total;
    if (total == 0 || total > cap || (!rows && !cols && !values)) return GENPHI_OK;

    const size_t list_bytes = al256(static_cast<size_t>(total) * 4);
    rc = scratch_for(p, off_bytes + 3 * list_bytes, "genphi_result_over", "the list of pairs (12 bytes each)", &scratch);
    if (rc) return rc;
    long long *d_off = reinterpret_cast<long long *>(scratch);
    int *d_row = reinterpret_cast<int *>(scratch + off_bytes), *d_col = reinterpret_cast<int *>(scratch + off_bytes + list_bytes);
    float *d_val = reinterpret_cast<float *>(scratch + off_bytes + 2 * list_bytes);
    static_assert(sizeof(long long) == sizeof(int64_t), "the offsets are uploaded as they are");
    hipError_t e = hipMemcpyAsync(d_off, oc.off.data(), static_cast<size_t>(nr + 1) * sizeof(long long), hipMemcpyHostToDevice, v.stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(over_write_kernel, dim3(static_cast<unsigned>(nr)), dim3(256), 0, v.stream, v.result, ld, n, r0, threshold,
                           d_off, static_cast<long long>(total), d_row, d_col, d_val);
        e = hipGetLastError();
    }
    const size_t out_bytes = static_cast<size_t>(total) * 4;
    return copy_back(v, e, {{rows, d_row, out_bytes}, {cols, d_col, out_bytes}, {values, d_val, out_bytes}}, "genphi_result_over");
}

// gen.phiCI: the bootstrap resamples' quadratic forms over the resident rows; the kernels are in bootstrap.hip.
int genphi_result_bootstrap(genphi_plan *p, uint64_t seed, int32_t first, int32_t n_boot, double *quad, double *self, int64_t *n_rows)
{
    if (!p) return genphi_set_error(GENPHI_ERR_ARG, "plan is NULL");
    const ResidentView v = genphi::resident_view(p);
    if (n_rows) *n_rows = v.n_rows;
    if (n_boot < 1 || first < 0 || first > INT32_MAX - n_boot)
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_result_bootstrap: resamples first = " + std::to_string(first) + ", n_boot = " + std::to_string(n_boot) +
                                                    " (need first >= 0, n_boot >= 1, first + n_boot < 2^31)");
    const int64_t N = v.n_pro, nr = v.n_rows;
    if (N < 2) return genphi_set_error(GENPHI_ERR_ARG, "genphi_result_bootstrap: a resample needs at least 2 probands, the plan has " + std::to_string(N));
    bool empty;
    int rc = need_f32_result(v, "genphi_result_bootstrap", kPhiMatrix, &empty);
    if (rc) return rc;
    if (empty) {                                        // an empty shard adds nothing
        if (quad) std::fill(quad, quad + n_boot, 0.0);
        if (self) std::fill(self, self + n_boot, 0.0);
        return GENPHI_OK;
    }
    if (v.ld < N || v.ld % 64 != 0) return genphi_set_error(GENPHI_ERR_DEVICE, "genphi_result_bootstrap: unexpected row pitch " + std::to_string(v.ld));
    SET_DEVICE(v);
    genphi::BootLaunch L;
    L.stream = v.stream;
    L.phi = v.result; L.ld = static_cast<long long>(v.ld);
    L.n = static_cast<int>(N); L.row_begin = static_cast<int>(v.row_begin); L.n_rows = static_cast<int>(nr);
    L.seed = seed; L.first = first; L.n_boot = n_boot;
    L.panel = genphi::boot_panel(L.n, n_boot, v.tun->boot_panel);
    L.quad = quad; L.self = self;
    rc = scratch_for(p, genphi::boot_scratch_bytes(L.n, L.n_rows, n_boot, L.panel), "genphi_result_bootstrap",
                     "the counts and partial sums of a panel of " + std::to_string(L.panel) + " resamples", &L.scratch);
    if (rc) return rc;
    const hipError_t e = genphi::boot_launch(L);
    if (e != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string("genphi_result_bootstrap: ") + hipGetErrorString(e));
    return GENPHI_OK;
}

// gen.phiNearest: one launch, a workgroup per resident row, into two n_rows x k arrays in the plan's scratch block ->
// one copy per array the caller asked for.
int genphi_result_nearest(genphi_plan *p, int32_t k, int32_t *cols, float *values)
{
    if (!p) return genphi_set_error(GENPHI_ERR_ARG, "plan is NULL");
    const ResidentView v = genphi::resident_view(p);
    if (!cols && !values) return genphi_set_error(GENPHI_ERR_ARG, "genphi_result_nearest: cols and values are both NULL");
    const int64_t N = v.n_pro, nr = v.n_rows;
    if (N < 2) return genphi_set_error(GENPHI_ERR_ARG, "genphi_result_nearest: " + std::to_string(N) + " probands have no nearest relative");
    if (k < 1 || k > std::min<int64_t>(N - 1, GENPHI_NEAREST_MAX_K))
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_result_nearest: k = " + std::to_string(k) + " outside [1, " +
                                                    std::to_string(std::min<int64_t>(N - 1, GENPHI_NEAREST_MAX_K)) + "]");
    bool empty;
    int rc = need_f32_result(v, "genphi_result_nearest", kPhiMatrix, &empty);
    if (rc || empty) return rc;
    SET_DEVICE(v);
    const size_t out_bytes = static_cast<size_t>(nr) * static_cast<size_t>(k) * 4, arr_bytes = al256(out_bytes);
    char *scratch;
    rc = scratch_for(p, 2 * arr_bytes, "genphi_result_nearest", "the output (8 bytes per row and neighbour)", &scratch);
    if (rc) return rc;
    int *d_col = reinterpret_cast<int *>(scratch);
    float *d_val = reinterpret_cast<float *>(scratch + arr_bytes);
    const int cap = v.tun->nearest_buf;
    hipLaunchKernelGGL(nearest_kernel, dim3(static_cast<unsigned>(nr)), dim3(256), static_cast<size_t>(cap) * sizeof(unsigned long long), v.stream,
                       v.result, static_cast<long long>(v.ld), static_cast<int>(N), static_cast<int>(v.row_begin), static_cast<int>(k), cap,
                       cols ? d_col : nullptr, values ? d_val : nullptr);
    return copy_back(v, hipGetLastError(), {{cols, d_col, out_bytes}, {values, d_val, out_bytes}}, "genphi_result_nearest");
}

// Group sums of the resident result: validate, the host tables (group_tables.h), one upload, the launches of
// group_tiles_kernel and of every level of group_rows_reduce_kernel, one copy of the n_groups x (n_groups + 1) table back.
// Everything lives in the plan's scratch block.
int genphi_result_group_sums(genphi_plan *p, int32_t n_groups, const int32_t *group, double *sums, double *diag,
                             int64_t *rows_in_group, int64_t *cols_in_group, int32_t *form_out)
{
    if (!p) return genphi_set_error(GENPHI_ERR_ARG, "plan is NULL");
    const ResidentView v = genphi::resident_view(p);
    if (n_groups < 1 || n_groups > kGsMaxGroups)
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_result_group_sums: n_groups = " + std::to_string(n_groups) + " outside [1, " +
                                                    std::to_string(kGsMaxGroups) + "] (GENPHI_GROUP_SUMS_MAX_GROUPS)");
    const int64_t N = v.n_pro;
    if (N > 0 && !group) return genphi_set_error(GENPHI_ERR_ARG, "genphi_result_group_sums: group is NULL");
    for (int64_t i = 0; i < N; ++i)
        if (group[i] < -1 || group[i] >= n_groups)
            return genphi_set_error(GENPHI_ERR_ARG, "genphi_result_group_sums: label " + std::to_string(group[i]) + " of proband " + std::to_string(i) +
                                                        " outside [-1, " + std::to_string(n_groups) + ")");
    if (v.res_f64 || N > 0) {                         // (no proband: nothing to be resident) an empty shard adds nothing, as for the other
        bool empty;                                   // queries: zeros, the column counts, the form
        const int rc = need_f32_result(v, "genphi_result_group_sums", kPhiMeanInput, &empty);
        if (rc) return rc;
    }
    const int G = n_groups, W = G + 1;
    const int64_t r0 = v.row_begin;
    genphi::GroupTables t;
    genphi::build_group_tables(group, G, N, r0, N > 0 ? v.n_rows : 0, v.n_cus, t);
    auto deliver = [&](const double *tab) {           // tab: G x W (sums | diag), or NULL = zeros
        for (int a = 0; a < G; ++a) {
            if (sums) for (int b = 0; b < G; ++b) sums[static_cast<size_t>(a) * G + b] = tab ? tab[static_cast<size_t>(a) * W + b] : 0.0;
            if (diag) diag[a] = tab ? tab[static_cast<size_t>(a) * W + G] : 0.0;
            if (rows_in_group) rows_in_group[a] = t.n_rows[a];
            if (cols_in_group) cols_in_group[a] = t.n_cols[a];
        }
        if (form_out) *form_out = t.form;
    };
    if (t.blocks.empty()) { deliver(nullptr); return GENPHI_OK; }
    if (t.n_part > INT32_MAX / 2) return genphi_set_error(GENPHI_ERR_ARG, "genphi_result_group_sums: too many row blocks");
    // one blob of tables, then part and the two buffers of the reduction
    std::vector<char> blob;
    auto put = [&](const void *src, size_t bytes) {
        const size_t off = blob.size();
        blob.resize(off + al256(std::max<size_t>(bytes, 1)));
        if (bytes) std::memcpy(blob.data() + off, src, bytes);
        return off;
    };
    static_assert(sizeof(genphi::GsPair) == sizeof(int2), "the pairs are uploaded as they are");
    const size_t o_rows = put(t.rowlist.data(), t.rowlist.size() * sizeof(int));
    const size_t o_blocks = put(t.blocks.data(), t.blocks.size() * sizeof(int2));
    const size_t o_tiles = put(t.tile_lists.data(), t.tile_lists.size() * sizeof(int2));
    const size_t o_a = put(t.list_a.data(), t.list_a.size() * sizeof(int));
    const size_t o_b = put(t.list_b.data(), t.list_b.size() * sizeof(int2));
    const size_t o_perm = put(t.perm.data(), t.perm.size() * sizeof(unsigned short));
    std::vector<size_t> o_beg;
    for (const auto &beg : t.level_beg) o_beg.push_back(put(beg.data(), beg.size() * sizeof(int)));
    size_t buf_rows[2] = {0, 0};
    for (size_t l = 0; l < t.level_rows.size(); ++l) buf_rows[l & 1] = std::max(buf_rows[l & 1], static_cast<size_t>(t.level_rows[l]));
    const size_t o_part = blob.size();
    const size_t o_buf0 = o_part + al256(static_cast<size_t>(t.n_part) * W * sizeof(double));
    const size_t o_buf1 = o_buf0 + al256(buf_rows[0] * W * sizeof(double));
    const size_t total = o_buf1 + al256(buf_rows[1] * W * sizeof(double));

    SET_DEVICE(v);
    char *d;
    const int rc = genphi::resident_scratch(p, total, &d);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(d, blob.data(), blob.size(), hipMemcpyHostToDevice, v.stream);
    std::vector<double> tab(static_cast<size_t>(G) * W);
    const double *in = nullptr;
    if (e == hipSuccess) {
        double *part = reinterpret_cast<double *>(d + o_part);
        double *buf[2] = {reinterpret_cast<double *>(d + o_buf0), reinterpret_cast<double *>(d + o_buf1)};
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(t.n_part)), dim3(256), 0, v.stream, v.result,
                               static_cast<long long>(v.ld), static_cast<int>(r0), reinterpret_cast<const int *>(d + o_rows),
                               reinterpret_cast<const int2 *>(d + o_blocks), reinterpret_cast<const int2 *>(d + o_tiles),
                               reinterpret_cast<const int *>(d + o_a), reinterpret_cast<const int2 *>(d + o_b),
                               reinterpret_cast<const unsigned short *>(d + o_perm), t.n_tiles, t.tiles_per_slab, t.n_slabs, G, part);
        };
        if (t.form) launch(group_tiles_kernel<true>);
        else launch(group_tiles_kernel<false>);
        e = hipGetLastError();
        in = part;
        for (size_t l = 0; l < t.level_rows.size() && e == hipSuccess; ++l) {
            hipLaunchKernelGGL(group_rows_reduce_kernel, dim3(static_cast<unsigned>(t.level_rows[l]), static_cast<unsigned>((W + 255) / 256)),
                               dim3(256), 0, v.stream, in, buf[l & 1], reinterpret_cast<const int *>(d + o_beg[l]), W);
            e = hipGetLastError();
            in = buf[l & 1];
        }
    }
    const int rc2 = copy_back(v, e, {{tab.data(), in, tab.size() * sizeof(double)}}, "genphi_result_group_sums");      // (the blob is read until here)
    if (rc2) return rc2;
    deliver(tab.data());
    return GENPHI_OK;
}

int genphi_result_entries(genphi_plan *p, int64_t n, const int64_t *rows, const int64_t *cols, double *out)
{
    if (!p) return genphi_set_error(GENPHI_ERR_ARG, "plan is NULL");
    const ResidentView v = genphi::resident_view(p);
    if (n < 0 || (n > 0 && (!rows || !cols || !out))) return genphi_set_error(GENPHI_ERR_ARG, "genphi_result_entries: bad argument");
    if (n == 0) return GENPHI_OK;
    if (!v.on_device || !(v.res_f64 ? static_cast<const void *>(v.result64) : static_cast<const void *>(v.result)))
        return genphi_set_error(GENPHI_ERR_DEVICE, "no resident result: call genphi_compute_device first");
    const int64_t N = v.n_pro, r0 = v.row_begin, nr = v.n_rows;
    std::vector<long long> off(static_cast<size_t>(n));
    for (int64_t k = 0; k < n; ++k) {
        if (rows[k] < r0 || rows[k] >= r0 + nr || cols[k] < 0 || cols[k] >= N)
            return genphi_set_error(GENPHI_ERR_ARG, "genphi_result_entries: entry (" + std::to_string(rows[k]) + ", " + std::to_string(cols[k]) +
                                                        ") outside the resident rows [" + std::to_string(r0) + ", " + std::to_string(r0 + nr) + ") x [0, " + std::to_string(N) + ")");
        off[k] = static_cast<long long>(rows[k] - r0) * v.ld + cols[k];
    }
    SET_DEVICE(v);
    const size_t off_bytes = al256(static_cast<size_t>(n) * sizeof(long long));
    char *scratch;
    const int rc = genphi::resident_scratch(p, off_bytes + static_cast<size_t>(n) * sizeof(double), &scratch);
    if (rc) return rc;
    long long *d_off = reinterpret_cast<long long *>(scratch);
    double *d_val = reinterpret_cast<double *>(scratch + off_bytes);
    hipError_t e = hipMemcpyAsync(d_off, off.data(), n * sizeof(long long), hipMemcpyHostToDevice, v.stream);
    if (e == hipSuccess) {
        if (v.res_f64)
            hipLaunchKernelGGL(gather_entries64_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, v.stream,
                               v.result64, d_off, n, d_val);
        else
            hipLaunchKernelGGL(gather_entries_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, v.stream,
                               v.result, d_off, n, d_val);
        e = hipGetLastError();
    }
    return copy_back(v, e, {{out, d_val, n * sizeof(double)}}, "genphi_result_entries");
}

}  // extern "C"
