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

#include "implex.h"
#include "sweep_device.h"

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

// gc's rule (sweep_panels.h): the rows of one panel within about 150 MiB, so that the rows a step writes are still in the 256 MiB
// Infinity Cache when the next step and the count read them.  Sized here, in words of 64 probands: a panel is three buffers and
// by default a power of two wide.
constexpr int64_t kMaxPanelWords = 1 << 20;

}  // namespace

struct genphi_implex : SweepDevice {         // d_slots: per panel of a launch: buffer 0, buffer 1, the seen matrix
    genphi::ImplexPlan plan;                 // host plan (implex.h)
    bool only_new = false;
    int32_t panel_env = 0, group_env = 0;    // GENPHI_IMPLEX_PANEL / GENPHI_IMPLEX_PANELS_PER_LAUNCH (0 = default rule)
    DevBuf<long long> d_counts;              // n_pro x G
    DevBuf<double> d_result;                 // n_pro x G percentages
    DevBuf<u64> d_totals;                    // G, on request
    DevBuf<int> d_occ_start, d_occ_cols, d_estart, d_child, d_seen_row;
    bool totals_ready = false;
    int32_t panel_cols = 0, lanes_per_row = 0;
    int64_t n_panels = 0;
    genphi_implex() { own(d_counts, d_result, d_totals, d_occ_start, d_occ_cols, d_estart, d_child, d_seen_row); }
    size_t result_entries() const { return static_cast<size_t>(plan.n_pro) * static_cast<size_t>(plan.G); }
    bool empty() const { return plan.n_pro == 0 || plan.G == 0; }
};

namespace {

int compute_impl(genphi_implex *h, int32_t device)
{
    if (int rc = h->select(device)) return rc;
    h->totals_ready = false;
    const genphi::ImplexPlan &pl = h->plan;
    const int G = pl.G;
    const int64_t n_pro = pl.n_pro;
    const size_t n_res = h->result_entries();
    double usable = 0.0;
    if (int rc = h->usable_bytes(usable, h->d_counts.get() ? 16 * n_res : 0)) return rc;
    const double list_bytes = 4.0 * static_cast<double>(pl.occ_start.size() + pl.occ_cols.size() + pl.edge_start.size() + pl.child.size() + pl.seen_row.size());
    const double room = usable - 16.0 * static_cast<double>(n_res) - (h->d_child.get() ? 0.0 : list_bytes) - (64 << 20);
    // panels: W words (64 columns each) per row, at a pitch of whole 16-byte pairs
    const int64_t panel_rows = 2 * pl.peak_rows + (h->only_new ? pl.n_union : 0);
    auto panel_bytes = [&](int64_t w) { return 8.0 * static_cast<double>(panel_rows) * static_cast<double>((w + 1) & ~int64_t(1)); };
    const int64_t needed = (n_pro + 63) / 64;
    int64_t W;
    if (h->panel_env > 0) {
        W = std::min<int64_t>((static_cast<int64_t>(h->panel_env) + 63) / 64, kMaxPanelWords);       // (not cut to the probands: a test forces a kernel form by it)
    } else {
        const int64_t budget = std::max<int64_t>(1, static_cast<int64_t>(genphi::kPanelSlotBytes / (8.0 * static_cast<double>(panel_rows))));
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
    GENPHI_HIP_TRY(h->d_slots.reserve(static_cast<size_t>(group) * static_cast<size_t>(panel_stride) * sizeof(u64)));
    GENPHI_HIP_TRY(h->d_totals.reserve(static_cast<size_t>(G)));
    GENPHI_HIP_TRY(h->d_counts.reserve(n_res));
    GENPHI_HIP_TRY(h->d_result.reserve(n_res));
    int rc;
    if ((rc = h->upload(h->d_occ_start, pl.occ_start)) || (rc = h->upload(h->d_occ_cols, pl.occ_cols)) ||
        (rc = h->upload(h->d_estart, pl.edge_start)) || (rc = h->upload(h->d_child, pl.child)) ||
        (h->only_new && (rc = h->upload(h->d_seen_row, pl.seen_row))))
        return rc;
    const int lpr = lanes_per_row(P);                         // step: lanes per row, one 16-byte pair each
    const int wpr = lanes_per_row(static_cast<int>(W));       // count: words of a row per group
    h->panel_cols = static_cast<int32_t>(C);
    h->lanes_per_row = lpr;
    h->n_panels = n_panels;
    SweepRun run;
    if ((rc = run.begin(*h, 0.0))) return rc;
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_counts, 0, h->d_counts.bytes(), h->stream));
    const int step_rows = 4 * (64 / lpr), count_rows = (256 / wpr) * IMPLEX_COUNT_ROWS;
    u64 *rows = h->slots<u64>();
    u64 *seen = h->only_new ? rows + 2 * buf_words : nullptr;
    for (int64_t g0 = 0; g0 < n_panels; g0 += group) {
        const unsigned np = static_cast<unsigned>(std::min<int64_t>(group, n_panels - g0));
        for (int g = 0; g < G; ++g) {
            const int n_rows = static_cast<int>(pl.rows[g]);
            u64 *cur = rows + (g & 1) * buf_words;
            const u64 *prev = rows + ((g & 1) ^ 1) * buf_words;
            if (g == 0) {
                const dim3 grid(static_cast<unsigned>((static_cast<long long>(n_rows) * Wp + 255) / 256), np);
                implex_init_kernel<<<grid, 256, 0, h->stream>>>(h->d_occ_start, h->d_occ_cols, n_rows, cur, panel_stride, Wp, static_cast<int>(C),
                                                                static_cast<int>(g0), h->d_seen_row, seen, panel_stride);
            } else {
                const dim3 grid(static_cast<unsigned>((n_rows + step_rows - 1) / step_rows), np);
                const int *es = h->d_estart + pl.start_begin[g], *ch = h->d_child + pl.child_begin[g];
                const int *sr = h->only_new ? h->d_seen_row + pl.row_begin[g] : nullptr;
                if (h->only_new) {
                    GENPHI_LPR_SWITCH(lpr, (implex_step_kernel<LPR, true><<<grid, 256, 0, h->stream>>>(
                                               es, ch, n_rows, reinterpret_cast<const ulonglong2 *>(prev), reinterpret_cast<ulonglong2 *>(cur),
                                               panel_stride / 2, P, sr, reinterpret_cast<ulonglong2 *>(seen), panel_stride / 2)));
                } else {
                    GENPHI_LPR_SWITCH(lpr, (implex_step_kernel<LPR, false><<<grid, 256, 0, h->stream>>>(
                                               es, ch, n_rows, reinterpret_cast<const ulonglong2 *>(prev), reinterpret_cast<ulonglong2 *>(cur),
                                               panel_stride / 2, P, nullptr, nullptr, 0)));
                }
            }
            GENPHI_HIP_TRY(hipGetLastError());
            const dim3 cgrid(static_cast<unsigned>((n_rows + count_rows - 1) / count_rows), static_cast<unsigned>((W + wpr - 1) / wpr), np);
            GENPHI_LPR_SWITCH(wpr, (implex_count_kernel<LPR><<<cgrid, 256, 0, h->stream>>>(cur, n_rows, panel_stride, Wp, static_cast<int>(C),
                                                                                          static_cast<int>(n_pro), static_cast<int>(g0), G, g,
                                                                                          reinterpret_cast<u64 *>(h->d_counts.get()))));
            GENPHI_HIP_TRY(hipGetLastError());
        }
    }
    implex_finish_kernel<<<static_cast<unsigned>((n_res + 255) / 256), 256, 0, h->stream>>>(h->d_counts, static_cast<long long>(n_res), G, h->d_result);
    GENPHI_HIP_TRY(hipGetLastError());
    run.bytes = 8.0 * static_cast<double>(W) * static_cast<double>(n_panels) * static_cast<double>(pl.sum_rows + pl.sum_edges);
    return run.end(*h);
}

}  // namespace

extern "C" {

int genphi_implex_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                         const int64_t *pro_ids, int32_t flags, genphi_implex **out)
{
    if (out) *out = nullptr;
    if (out && (flags & ~GENPHI_IMPLEX_FLAG_ONLY_NEW)) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_create: unknown flag");
    if (int rc = check_create_args("genphi_implex_create", n_ind, ind, father, mother, n_pro, pro_ids, 0, nullptr, out, 0)) return rc;
    return create_entry(out, "gen.implex", [&](genphi_implex *h) {
        h->only_new = (flags & GENPHI_IMPLEX_FLAG_ONLY_NEW) != 0;
        h->panel_env = hook_count("GENPHI_IMPLEX_PANEL");
        h->group_env = hook_count("GENPHI_IMPLEX_PANELS_PER_LAUNCH");
        std::string err;
        if (const int rc = genphi::plan_implex(h->plan, n_ind, ind, father, mother, n_pro, pro_ids, GENPHI_IMPLEX_MAX_GENERATIONS, err))
            return genphi_set_error(rc, err);
        if (h->plan.seen_row.size() + static_cast<size_t>(h->plan.G) >= static_cast<size_t>(INT32_MAX) || h->plan.child.size() >= static_cast<size_t>(INT32_MAX))
            return genphi_set_error(GENPHI_ERR_ALLOC, "gen.implex: the frontier lists of " + std::to_string(h->plan.G) + " generations exceed 2^31 entries");
        return GENPHI_OK;
    });
}

int genphi_implex_compute(genphi_implex *h, int32_t device) { return compute_entry(h, device, "genphi_implex_compute", "gen.implex", compute_impl); }

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
    return h->copy_out(out, h->d_counts, h->d_counts.bytes(), "gen.implex");
}

int genphi_implex_result_to_host(genphi_implex *h, double *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_result_to_host: nothing computed");
    if (h->empty()) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_result_to_host: out is NULL");
    return h->copy_out(out, h->d_result, h->d_result.bytes(), "gen.implex");
}

int genphi_implex_totals(genphi_implex *h, int64_t *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_totals: nothing computed");
    if (h->empty()) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_totals: out is NULL");
    const size_t bytes = static_cast<size_t>(h->plan.G) * sizeof(int64_t);
    if (!h->totals_ready) {
        const int rc = h->on_device("gen.implex totals", [&] {
            const hipError_t e = hipMemsetAsync(h->d_totals, 0, bytes, h->stream);
            if (e != hipSuccess) return e;
            implex_colsum_kernel<<<static_cast<unsigned>((h->plan.n_pro + 1023) / 1024), 256, 0, h->stream>>>(h->d_counts, h->plan.n_pro, h->plan.G, h->d_totals);
            return hipGetLastError();
        });
        if (rc) return rc;
        h->totals_ready = true;
    }
    return h->copy_out(out, h->d_totals, bytes, "gen.implex");
}

int genphi_implex_stats(const genphi_implex *h, double *sweep_ms, double *algorithmic_bytes, int32_t *generations, int32_t *panel_cols,
                        int64_t *panels, int32_t *lanes_per_row, int64_t *peak_rows)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_implex_stats: NULL handle");
    h->stats(sweep_ms, algorithmic_bytes, nullptr);
    put(generations, h->plan.G);
    put(panel_cols, h->panel_cols);
    put(panels, h->n_panels);
    put(lanes_per_row, h->lanes_per_row);
    put(peak_rows, h->plan.peak_rows);
    return GENPHI_OK;
}

void genphi_implex_destroy(genphi_implex *h) { destroy_entry(h); }

}  // extern "C"
