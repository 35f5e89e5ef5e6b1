// implex.hip -- gen.implex: the DISTINCT ancestors of every proband per generation (include/genphi.h, genphi_implex_*).
//
// GENLIB's gen.implex (the reference has no form of it): A_0(p) = {p}, A_{g+1}(p) = the known parents of the members of A_g(p);
// counts[i][g] = |A_g(pro[i])|, or -- GENPHI_IMPLEX_FLAG_ONLY_NEW -- |A_g \ (A_0 u .. u A_{g-1})|, the individuals whose shortest
// ascent from the proband has g meioses.  Entry = count / 2^g * 100.
//
// Here: a level-synchronous frontier over bit rows, walked upwards from the probands.  Rows are individuals, columns are the listed
// probands as bits, 64 per word: bit i of the row of x in generation g says "x is in A_g(pro[i])".  The host plan (implex.h, no
// GPU) lists per generation the union frontier U_g and, per row of U_g, the positions in U_{g-1} of its children:
//     row_g[x] = OR over the children c of x in U_{g-1} of row_{g-1}[c]
//     only new: row_g[x] &= ~seen[x];  seen[x] |= row_g[x]       (a breadth-first search with a visited set: the parents of an
//                                                                 individual that was seen before are never new)
// Frontier rows live in two compact buffers indexed by position in U_g, read and written in turn: a step reads only rows that the
// step before wrote, and nothing is cleared between generations.  The seen matrix is indexed by position in the union of all
// U_g; the generation that meets an individual first writes its seen row instead of reading it, so it is not cleared either.
//   step    one launch per generation and panel group: LPR lanes per row (a power of two), 16 bytes per lane and access, the
//           child list walked in a loop of any length with four rows in flight
//   count   one launch per generation and panel group, after the step: per proband column, the rows of U_g whose bit is set.  A
//           lane owns one word of the rows it walks (at most 255 of them) and adds them into eight bit planes (a ripple-carry
//           counter per bit: 24 operations per word instead of 128 for 64 separate counters); the planes are expanded once, the
//           groups of a block are combined in LDS, and one 64-bit integer atomic per column and block goes to counts[i * G + g].
//           Each (proband, g) belongs to one panel and one step, integer addition is associative: the same bits on every run.
//   finish  one kernel writes the percentages next to the counts by (double)count / 2^g * 100.0 (-ffp-contract=off)
//   totals  column sums of the resident counts on the device (as gen.completeness), on request
// Column panels: the columns are independent; the probands are swept in panels of a multiple of 64 columns, by default as wide
// as keeps one panel's two frontier buffers (and its seen matrix) within about 150 MiB (gc's rule).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "../../include/genphi.h"
#include "devcache.h"
#include "implex.h"
#include "planner.h"

int genphi_set_error(int code, const std::string &msg);      // genphi_hip.hip

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ ulonglong2 or2(ulonglong2 a, const ulonglong2 b)
{
    a.x |= b.x; a.y |= b.y;
    return a;
}

// U_0: row r = the bits of the listed occurrences of its proband that fall into the panel; a thread per word of a row (the
// padding word of an odd row width included: the steps move whole 16-byte pairs).  Every row of U_0 is met for the first time:
// its seen row is written.
__global__ void __launch_bounds__(256)
implex_init_kernel(const int *__restrict__ occ_start, const int *__restrict__ occ_cols, int n_rows, u64 *__restrict__ buf,
                   long long panel_stride, int Wp, int C, int panel0, const int *__restrict__ seen_row, u64 *__restrict__ seen,
                   long long seen_stride)
{
    const long long t = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const long long row = t / Wp;
    if (row >= n_rows) return;
    const int w = static_cast<int>(t % Wp);
    const long long p0 = static_cast<long long>(panel0 + static_cast<int>(blockIdx.y)) * C;
    u64 word = 0;
    for (int k = occ_start[row]; k < occ_start[row + 1]; ++k) {
        const long long c = occ_cols[k] - p0;
        if (c >= 0 && c < C && (c >> 6) == w) word |= 1ull << (c & 63);
    }
    buf[static_cast<long long>(blockIdx.y) * panel_stride + row * Wp + w] = word;
    if (seen) seen[static_cast<long long>(blockIdx.y) * seen_stride + static_cast<long long>(~seen_row[row]) * Wp + w] = word;
}

// One row of U_g = the OR of the rows of its children in U_{g-1}.  LPR lanes per row (a power of two), lane l moves the 16-byte
// pairs l, l + LPR, ..; a wave holds 64 / LPR rows.  All sizes in pairs (two words).
template <int LPR, bool ONLY_NEW>
__global__ void __launch_bounds__(256)
implex_step_kernel(const int *__restrict__ estart, const int *__restrict__ child, int n_rows, const ulonglong2 *__restrict__ prev,
                   ulonglong2 *__restrict__ cur, long long panel_stride, int P, const int *__restrict__ seen_row,
                   ulonglong2 *__restrict__ seen, long long seen_stride)
{
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (static_cast<long long>(blockIdx.x) * 4 + wave) * RPW + lane / LPR;
    if (row >= n_rows) return;
    const int l = lane % LPR;
    const int eb = estart[row], ee = estart[row + 1];
    prev += static_cast<long long>(blockIdx.y) * panel_stride;
    cur += static_cast<long long>(blockIdx.y) * panel_stride;
    for (int c = l; c < P; c += LPR) {
        ulonglong2 acc = make_ulonglong2(0, 0);
        int e = eb;
        for (; e + 4 <= ee; e += 4) {
            const ulonglong2 a0 = prev[static_cast<long long>(child[e]) * P + c];
            const ulonglong2 a1 = prev[static_cast<long long>(child[e + 1]) * P + c];
            const ulonglong2 a2 = prev[static_cast<long long>(child[e + 2]) * P + c];
            const ulonglong2 a3 = prev[static_cast<long long>(child[e + 3]) * P + c];
            acc = or2(or2(acc, or2(a0, a1)), or2(a2, a3));
        }
        for (; e < ee; ++e) acc = or2(acc, prev[static_cast<long long>(child[e]) * P + c]);
        if (ONLY_NEW) {
            const int s = seen_row[row];
            ulonglong2 *sp = seen + static_cast<long long>(blockIdx.y) * seen_stride + static_cast<long long>(s < 0 ? ~s : s) * P + c;
            if (s >= 0) {
                const ulonglong2 old = *sp;
                acc.x &= ~old.x; acc.y &= ~old.y;
                if (acc.x | acc.y) *sp = or2(old, acc);
            } else {
                *sp = acc;                         // met for the first time: nothing to read
            }
        }
        cur[row * P + c] = acc;
    }
}

// Per proband column, the rows of U_g whose bit is set.  LPR lanes per row here means LPR WORDS (a power of two): lane l of a
// group owns word blockIdx.y * LPR + l of the rows its group walks, 256 / LPR groups per block, block x owns
// IMPLEX_COUNT_ROWS * 256 / LPR consecutive rows and deals them round-robin to its groups (the lanes of a wave read neighbouring
// rows), so a group walks at most 255 rows: eight bit planes hold the count of every bit.
constexpr int IMPLEX_COUNT_ROWS = 255;

template <int LPR>
__global__ void __launch_bounds__(256)
implex_count_kernel(const u64 *__restrict__ cur, int n_rows, long long panel_stride, int Wp, int C, int n_pro, int panel0, int G,
                    int g, u64 *__restrict__ counts)
{
    constexpr int GPB = 256 / LPR;
    __shared__ unsigned sums[LPR * 64];
    for (int i = threadIdx.x; i < LPR * 64; i += 256) sums[i] = 0;
    __syncthreads();
    const int grp = threadIdx.x / LPR, l = threadIdx.x % LPR;
    const long long p0 = static_cast<long long>(panel0 + static_cast<int>(blockIdx.z)) * C;
    const int ncols = static_cast<int>(min(static_cast<long long>(C), n_pro - p0));
    const int nw = (ncols + 63) >> 6;
    const int w = static_cast<int>(blockIdx.y) * LPR + l;
    const long long r0 = static_cast<long long>(blockIdx.x) * (GPB * IMPLEX_COUNT_ROWS);
    const long long r1 = min(r0 + GPB * IMPLEX_COUNT_ROWS, static_cast<long long>(n_rows));
    if (w < nw && r0 + grp < r1) {
        const u64 *base = cur + static_cast<long long>(blockIdx.z) * panel_stride + w;
        u64 plane[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) plane[k] = 0;
#pragma unroll 4
        for (long long r = r0 + grp; r < r1; r += GPB) {
            u64 carry = base[r * Wp];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const u64 t = plane[k] & carry;
                plane[k] ^= carry;
                carry = t;
            }
        }
        u64 any = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) any |= plane[k];
        for (int b = 0; b < 64; ++b) {
            if (!((any >> b) & 1)) continue;
            unsigned cnt = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) cnt |= static_cast<unsigned>((plane[k] >> b) & 1) << k;
            atomicAdd(&sums[l * 64 + b], cnt);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < LPR * 64; i += 256) {
        const unsigned v = sums[i];
        const int j = (static_cast<int>(blockIdx.y) * LPR + i / 64) * 64 + (i & 63);
        if (v && j < ncols) atomicAdd(&counts[(p0 + j) * G + g], static_cast<u64>(v));
    }
}

// the percentages next to the counts: the two Float64 operations of gen.completeness, in its order
__global__ void __launch_bounds__(256)
implex_finish_kernel(const long long *__restrict__ counts, long long n, int G, double *__restrict__ pct)
{
    const long long o = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (o >= n) return;
    const int g = static_cast<int>(o % G);
    pct[o] = static_cast<double>(counts[o]) / static_cast<double>(1ull << g) * 100.0;
}

// Totals: column sums of the n_rows x G counts (lane g owns column g, the 4 waves of a block share 1,024 rows).
__global__ void __launch_bounds__(256)
implex_colsum_kernel(const long long *__restrict__ counts, long long n_rows, int G, u64 *__restrict__ totals)
{
    const int g = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (g >= G) return;
    const long long r0 = static_cast<long long>(blockIdx.x) * 1024, r1 = min(r0 + 1024, n_rows);
    u64 s = 0;
    for (long long r = r0 + wave; r < r1; r += 4) s += static_cast<u64>(counts[r * G + g]);
    if (s) atomicAdd(&totals[g], s);
}

#define IMPLEX_LPR_SWITCH(lpr, CALL)                   \
    switch (lpr) {                                     \
    case 1: { constexpr int LPR = 1; CALL; } break;    \
    case 2: { constexpr int LPR = 2; CALL; } break;    \
    case 4: { constexpr int LPR = 4; CALL; } break;    \
    case 8: { constexpr int LPR = 8; CALL; } break;    \
    case 16: { constexpr int LPR = 16; CALL; } break;  \
    case 32: { constexpr int LPR = 32; CALL; } break;  \
    default: { constexpr int LPR = 64; CALL; } break;  \
    }

// gc's rule (gc.hip): the rows of one panel within about 150 MiB, so that the rows a step writes are still in the 256 MiB
// Infinity Cache when the next step and the count read them.
constexpr double kPanelBytes = 150.0 * 1048576.0;
constexpr int64_t kMaxPanelWords = 1 << 20;

int pow2_at_least(int64_t n, int cap)
{
    int p = 1;
    while (p < n && p < cap) p *= 2;
    return p;
}

}  // namespace

struct genphi_implex {
    genphi::ImplexPlan plan;                 // host plan (implex.h)
    bool only_new = false;
    int32_t panel_env = 0, group_env = 0;    // GENPHI_IMPLEX_PANEL / GENPHI_IMPLEX_PANELS_PER_LAUNCH (0 = default rule)
    // device
    int device = -1;
    hipStream_t stream = nullptr;
    long long *d_counts = nullptr;           // n_pro x G
    double *d_result = nullptr;              // n_pro x G percentages
    u64 *d_totals = nullptr;                 // G, on request
    int *d_occ_start = nullptr, *d_occ_cols = nullptr, *d_estart = nullptr, *d_child = nullptr, *d_seen_row = nullptr;
    u64 *d_rows = nullptr;                   // per panel of a launch: buffer 0, buffer 1, the seen matrix
    size_t rows_bytes = 0;
    bool computed = false, totals_ready = false;
    double sweep_ms = 0.0, alg_bytes = 0.0;
    int32_t panel_cols = 0, lanes_per_row = 0;
    int64_t n_panels = 0;
    size_t result_entries() const { return static_cast<size_t>(plan.n_pro) * static_cast<size_t>(plan.G); }
    bool empty() const { return plan.n_pro == 0 || plan.G == 0; }
};

namespace {

void release_device(genphi_implex *h)
{
    if (h->device < 0) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    void *blocks[] = {h->d_counts, h->d_result, h->d_totals, h->d_occ_start, h->d_occ_cols, h->d_estart, h->d_child, h->d_seen_row, h->d_rows};
    for (void *p : blocks) (void)genphi::cached_free(p);
    h->d_counts = nullptr; h->d_result = nullptr; h->d_totals = nullptr; h->d_occ_start = nullptr; h->d_occ_cols = nullptr;
    h->d_estart = nullptr; h->d_child = nullptr; h->d_seen_row = nullptr; h->d_rows = nullptr; h->rows_bytes = 0;
    if (h->stream) genphi::cached_stream_release(h->stream, h->device);
    h->stream = nullptr;
    (void)hipSetDevice(cur);
    h->device = -1;
    h->computed = false; h->totals_ready = false;
}

#define IMPLEX_TRY(expr)                                                                                        \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

int upload(genphi_implex *h, int **dst, const std::vector<int32_t> &src)
{
    if (*dst || src.empty()) return GENPHI_OK;
    IMPLEX_TRY(genphi::cached_malloc(reinterpret_cast<void **>(dst), src.size() * sizeof(int32_t)));
    IMPLEX_TRY(hipMemcpyAsync(*dst, src.data(), src.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    return GENPHI_OK;
}

int compute_impl(genphi_implex *h, int32_t device)
{
    if (device < 0) IMPLEX_TRY(hipGetDevice(&device));
    if (h->device >= 0 && h->device != device) release_device(h);
    IMPLEX_TRY(hipSetDevice(device));
    h->device = device;
    h->computed = false; h->totals_ready = false;
    if (!h->stream) IMPLEX_TRY(genphi::cached_stream(&h->stream));
    const genphi::ImplexPlan &pl = h->plan;
    const int G = pl.G;
    const int64_t n_pro = pl.n_pro;
    const size_t n_res = h->result_entries();
    size_t free_b = 0, total_b = 0;
    IMPLEX_TRY(hipMemGetInfo(&free_b, &total_b));
    const double list_bytes = 4.0 * static_cast<double>(pl.occ_start.size() + pl.occ_cols.size() + pl.edge_start.size() + pl.child.size() + pl.seen_row.size());
    const double usable = 0.9 * static_cast<double>(free_b + h->rows_bytes + (h->d_counts ? 16 * n_res : 0));
    const double room = usable - 16.0 * static_cast<double>(n_res) - (h->d_child ? 0.0 : list_bytes) - (64 << 20);
    // panels: W words (64 columns each) per row, at a pitch of whole 16-byte pairs
    const int64_t panel_rows = 2 * pl.peak_rows + (h->only_new ? pl.n_union : 0);
    auto panel_bytes = [&](int64_t w) { return 8.0 * static_cast<double>(panel_rows) * static_cast<double>((w + 1) & ~int64_t(1)); };
    const int64_t needed = (n_pro + 63) / 64;
    int64_t W;
    if (h->panel_env > 0) {
        W = std::min<int64_t>((static_cast<int64_t>(h->panel_env) + 63) / 64, kMaxPanelWords);       // (not cut to the probands: a test forces a kernel form by it)
    } else {
        const int64_t budget = std::max<int64_t>(1, static_cast<int64_t>(kPanelBytes / (8.0 * static_cast<double>(panel_rows))));
        W = 1;
        while (2 * W <= budget && 2 * W <= kMaxPanelWords) W *= 2;                                     // a power of two: no idle lanes in a row
        W = std::min(W, needed);
        while (W > 1 && panel_bytes(W) > room) W = (W + 1) / 2;
    }
    if (panel_bytes(W) > room)
        return genphi_set_error(GENPHI_ERR_ALLOC, "gen.implex: " + std::to_string(panel_rows) + " frontier rows of " + std::to_string(64 * W) +
                                                      " columns do not fit on device " + std::to_string(device) + " beside the result");
    const int64_t C = 64 * W;
    const int64_t n_panels = (n_pro + C - 1) / C;
    int64_t group = 1;
    if (h->panel_env > 0) group = std::max<int64_t>(1, std::min<int64_t>(n_panels, static_cast<int64_t>(room / panel_bytes(W))));
    if (h->group_env > 0) group = h->group_env;
    group = std::max<int64_t>(1, std::min<int64_t>({group, n_panels, 65535, static_cast<int64_t>(room / panel_bytes(W))}));
    const int Wp = static_cast<int>((W + 1) & ~int64_t(1)), P = Wp / 2;
    const long long panel_stride = static_cast<long long>(panel_rows) * Wp;        // words of one panel: buffer 0, buffer 1, seen
    const long long buf_words = static_cast<long long>(pl.peak_rows) * Wp;
    const size_t need_rows = static_cast<size_t>(group) * static_cast<size_t>(panel_stride) * sizeof(u64);
    if (need_rows > h->rows_bytes) {
        (void)genphi::cached_free(h->d_rows);
        h->d_rows = nullptr; h->rows_bytes = 0;
        IMPLEX_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_rows), need_rows));
        h->rows_bytes = need_rows;
    }
    if (!h->d_totals) IMPLEX_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_totals), static_cast<size_t>(G) * sizeof(u64)));
    if (!h->d_counts) IMPLEX_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_counts), n_res * sizeof(long long)));
    if (!h->d_result) IMPLEX_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_result), n_res * sizeof(double)));
    int rc;
    if ((rc = upload(h, &h->d_occ_start, pl.occ_start)) || (rc = upload(h, &h->d_occ_cols, pl.occ_cols)) ||
        (rc = upload(h, &h->d_estart, pl.edge_start)) || (rc = upload(h, &h->d_child, pl.child)) ||
        (h->only_new && (rc = upload(h, &h->d_seen_row, pl.seen_row))))
        return rc;
    const int lpr = pow2_at_least(P, 64);                     // step: lanes per row, one 16-byte pair each
    const int wpr = pow2_at_least(W, 64);                     // count: words of a row per group
    h->panel_cols = static_cast<int32_t>(C);
    h->lanes_per_row = lpr;
    h->n_panels = n_panels;
    hipEvent_t e0, e1;
    IMPLEX_TRY(hipEventCreate(&e0));
    IMPLEX_TRY(hipEventCreate(&e1));
    IMPLEX_TRY(hipEventRecord(e0, h->stream));
    IMPLEX_TRY(hipMemsetAsync(h->d_counts, 0, n_res * sizeof(long long), h->stream));
    const int step_rows = 4 * (64 / lpr), count_rows = (256 / wpr) * IMPLEX_COUNT_ROWS;
    u64 *seen = h->only_new ? h->d_rows + 2 * buf_words : nullptr;
    for (int64_t g0 = 0; g0 < n_panels; g0 += group) {
        const unsigned np = static_cast<unsigned>(std::min<int64_t>(group, n_panels - g0));
        for (int g = 0; g < G; ++g) {
            const int n_rows = static_cast<int>(pl.rows[g]);
            u64 *cur = h->d_rows + (g & 1) * buf_words;
            const u64 *prev = h->d_rows + ((g & 1) ^ 1) * buf_words;
            if (g == 0) {
                const dim3 grid(static_cast<unsigned>((static_cast<long long>(n_rows) * Wp + 255) / 256), np);
                implex_init_kernel<<<grid, 256, 0, h->stream>>>(h->d_occ_start, h->d_occ_cols, n_rows, cur, panel_stride, Wp, static_cast<int>(C),
                                                                static_cast<int>(g0), h->d_seen_row, seen, panel_stride);
            } else {
                const dim3 grid(static_cast<unsigned>((n_rows + step_rows - 1) / step_rows), np);
                const int *es = h->d_estart + pl.start_begin[g], *ch = h->d_child + pl.child_begin[g];
                const int *sr = h->only_new ? h->d_seen_row + pl.row_begin[g] : nullptr;
                if (h->only_new) {
                    IMPLEX_LPR_SWITCH(lpr, (implex_step_kernel<LPR, true><<<grid, 256, 0, h->stream>>>(
                                               es, ch, n_rows, reinterpret_cast<const ulonglong2 *>(prev), reinterpret_cast<ulonglong2 *>(cur),
                                               panel_stride / 2, P, sr, reinterpret_cast<ulonglong2 *>(seen), panel_stride / 2)));
                } else {
                    IMPLEX_LPR_SWITCH(lpr, (implex_step_kernel<LPR, false><<<grid, 256, 0, h->stream>>>(
                                               es, ch, n_rows, reinterpret_cast<const ulonglong2 *>(prev), reinterpret_cast<ulonglong2 *>(cur),
                                               panel_stride / 2, P, nullptr, nullptr, 0)));
                }
            }
            IMPLEX_TRY(hipGetLastError());
            const dim3 cgrid(static_cast<unsigned>((n_rows + count_rows - 1) / count_rows), static_cast<unsigned>((W + wpr - 1) / wpr), np);
            IMPLEX_LPR_SWITCH(wpr, (implex_count_kernel<LPR><<<cgrid, 256, 0, h->stream>>>(cur, n_rows, panel_stride, Wp, static_cast<int>(C),
                                                                                         static_cast<int>(n_pro), static_cast<int>(g0), G, g,
                                                                                         reinterpret_cast<u64 *>(h->d_counts))));
            IMPLEX_TRY(hipGetLastError());
        }
    }
    implex_finish_kernel<<<static_cast<unsigned>((n_res + 255) / 256), 256, 0, h->stream>>>(h->d_counts, static_cast<long long>(n_res), G, h->d_result);
    IMPLEX_TRY(hipGetLastError());
    IMPLEX_TRY(hipEventRecord(e1, h->stream));
    IMPLEX_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    IMPLEX_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    h->sweep_ms = ms;
    h->alg_bytes = 8.0 * static_cast<double>(W) * static_cast<double>(n_panels) * static_cast<double>(pl.sum_rows + pl.sum_edges);
    h->computed = true;
    return GENPHI_OK;
}

// bytes from the device (src) to the host
int copy_out(genphi_implex *h, void *out, const void *src, size_t bytes)
{
    int cur = 0;
    IMPLEX_TRY(hipGetDevice(&cur));
    IMPLEX_TRY(hipSetDevice(h->device));
    const hipError_t e = hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, h->stream);
    const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(h->stream) : e;
    (void)hipSetDevice(cur);
    if (e2 != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string("gen.implex result copy: ") + hipGetErrorString(e2));
    return GENPHI_OK;
}

}  // namespace

extern "C" {

int genphi_implex_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                         const int64_t *pro_ids, int32_t flags, genphi_implex **out)
{
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_create: out is NULL");
    *out = nullptr;
    if (flags & ~GENPHI_IMPLEX_FLAG_ONLY_NEW) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_create: unknown flag");
    if (n_ind < 0 || n_pro < 0 || (n_ind && (!ind || !father || !mother)) || (n_pro && !pro_ids))
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_create: bad sizes or NULL arrays");
    if (n_ind >= INT32_MAX || n_pro >= INT32_MAX)
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_create: more than 2^31 - 2 individuals or probands");
    genphi_implex *h = new (std::nothrow) genphi_implex();
    if (!h) return genphi_set_error(GENPHI_ERR_ALLOC, "out of memory");
    h->only_new = (flags & GENPHI_IMPLEX_FLAG_ONLY_NEW) != 0;
    if (const char *e = genphi::env_hook("GENPHI_IMPLEX_PANEL")) h->panel_env = std::max(0, std::atoi(e));
    if (const char *e = genphi::env_hook("GENPHI_IMPLEX_PANELS_PER_LAUNCH")) h->group_env = std::max(0, std::atoi(e));
    int rc;
    try {
        std::string err;
        rc = genphi::plan_implex(h->plan, n_ind, ind, father, mother, n_pro, pro_ids, GENPHI_IMPLEX_MAX_GENERATIONS, err);
        if (rc) rc = genphi_set_error(rc, err);
        else if (h->plan.seen_row.size() + static_cast<size_t>(h->plan.G) >= static_cast<size_t>(INT32_MAX) || h->plan.child.size() >= static_cast<size_t>(INT32_MAX))
            rc = genphi_set_error(GENPHI_ERR_ALLOC, "gen.implex: the frontier lists of " + std::to_string(h->plan.G) + " generations exceed 2^31 entries");
    } catch (const std::bad_alloc &) { rc = genphi_set_error(GENPHI_ERR_ALLOC, "out of memory while planning gen.implex"); }
    if (rc) { delete h; return rc; }
    *out = h;
    return GENPHI_OK;
}

int genphi_implex_compute(genphi_implex *h, int32_t device)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_compute: NULL handle");
    if (h->empty()) { h->computed = true; h->sweep_ms = 0.0; h->alg_bytes = 0.0; return GENPHI_OK; }
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, "gen.implex: no usable GPU");
    int rc;
    try {
        rc = compute_impl(h, device);
    } catch (const std::bad_alloc &) { rc = genphi_set_error(GENPHI_ERR_ALLOC, "out of host memory in gen.implex"); }
    (void)hipSetDevice(cur);
    return rc;
}

int genphi_implex_generations(const genphi_implex *h, int32_t *generations)
{
    if (!h || !generations) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_generations: NULL argument");
    *generations = h->plan.G;
    return GENPHI_OK;
}

int genphi_implex_frontier_rows(const genphi_implex *h, int64_t *out)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_frontier_rows: NULL handle");
    if (h->plan.G && !out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_frontier_rows: out is NULL");
    for (int g = 0; g < h->plan.G; ++g) out[g] = h->plan.rows[g];
    return GENPHI_OK;
}

int genphi_implex_counts(genphi_implex *h, int64_t *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_counts: nothing computed");
    if (h->empty()) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_counts: out is NULL");
    return copy_out(h, out, h->d_counts, h->result_entries() * sizeof(long long));
}

int genphi_implex_result_to_host(genphi_implex *h, double *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_result_to_host: nothing computed");
    if (h->empty()) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_result_to_host: out is NULL");
    return copy_out(h, out, h->d_result, h->result_entries() * sizeof(double));
}

int genphi_implex_totals(genphi_implex *h, int64_t *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_totals: nothing computed");
    if (h->empty()) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_totals: out is NULL");
    const size_t bytes = static_cast<size_t>(h->plan.G) * sizeof(int64_t);
    if (!h->totals_ready) {
        int cur = 0;
        IMPLEX_TRY(hipGetDevice(&cur));
        IMPLEX_TRY(hipSetDevice(h->device));
        hipError_t e = hipMemsetAsync(h->d_totals, 0, bytes, h->stream);
        if (e == hipSuccess) {
            implex_colsum_kernel<<<static_cast<unsigned>((h->plan.n_pro + 1023) / 1024), 256, 0, h->stream>>>(h->d_counts, h->plan.n_pro, h->plan.G, h->d_totals);
            e = hipGetLastError();
        }
        (void)hipSetDevice(cur);
        if (e != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string("gen.implex totals: ") + hipGetErrorString(e));
        h->totals_ready = true;
    }
    return copy_out(h, out, h->d_totals, bytes);
}

int genphi_implex_stats(const genphi_implex *h, double *sweep_ms, double *algorithmic_bytes, int32_t *generations, int32_t *panel_cols,
                        int64_t *panels, int32_t *lanes_per_row, int64_t *peak_rows)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_stats: NULL handle");
    if (sweep_ms) *sweep_ms = h->sweep_ms;
    if (algorithmic_bytes) *algorithmic_bytes = h->alg_bytes;
    if (generations) *generations = h->plan.G;
    if (panel_cols) *panel_cols = h->panel_cols;
    if (panels) *panels = h->n_panels;
    if (lanes_per_row) *lanes_per_row = h->lanes_per_row;
    if (peak_rows) *peak_rows = h->plan.peak_rows;
    return GENPHI_OK;
}

void genphi_implex_destroy(genphi_implex *h)
{
    if (!h) return;
    release_device(h);
    delete h;
}

}  // extern "C"
