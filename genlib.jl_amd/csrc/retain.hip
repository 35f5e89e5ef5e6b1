// retain.hip -- gen.simuRetention: which founder alleles survive in the listed probands, by gene dropping (include/genphi.h,
// genphi_retain_*).  The label sweep is the shared one (label_sweep.h: the base of the handle, the init kernel and the step kernel, on
// ident's columns: row r, pair j, side s, plane b at ((r * Pn + j) * 2 + s) * B + b, 16-byte elements); the plan is ident.h's.
// Only the reduction is new, and it is the hot path:
//   mark    one launch per panel after the last level, grid (words of the panel, label chunks), 1,024 threads.  A workgroup owns the
//           64 simulations of one word and the labels [l0, l0 + LC) of one chunk (retain.h: retain_chunks).  It holds 64 bitmaps in
//           LDS, one per simulation, of LC + 1 bits: bit LC is the halo, label l0 + LC, so that a founder whose two labels straddle
//           a chunk border still gets its `both`.  Lane s of every wave is simulation s: the lanes of a wave never meet in one LDS
//           word, only waves do, and those are resolved by 32-bit LDS atomicOr.  The bitmaps lie stride dwords apart, stride odd:
//           for one label the 64 lanes fall on 64 different banks.
//           1. zero the bitmaps.
//           2. mark: wave v takes the sides u = v, v + 16, .. < 2 n_pro (proband u >> 1, side u & 1), read in place through pro_row
//              (there is no gather).  Lane b < B loads its word's half of plane b, one 8-byte load per lane; the label of lane s
//              is then bit s of the B words, which reach every lane as wave-uniform values (readlane).  Four sides are loaded
//              before the first is decoded.  A column < S whose label lies in [l0, l0 + LC] sets its bit.
//           3. reduce, after a barrier, the dwords of the bitmaps dealt to the waves: lane s reads dword d of its own bitmap.
//              distinct: popcounts, halo excluded, one atomicAdd per wave and column.  survived: per label a wave ballot of its bit
//              masked to the columns < S, then popcount; the counts of the 32 labels of a dword go out as one coalesced atomicAdd of
//              32 lanes.  both: popcount of ballot(l) & ballot(l + 1) where const_side[l] >> 1 == const_side[l + 1] >> 1 (the same
//              row, hence the same individual); bit 32 of the walk is bit 0 of the next dword, the halo at the chunk's end.
// Everything is integer; the only atomics on global memory are integer adds: the same bytes on every run, with any panel and chunk.
#include <hip/hip_runtime.h>

#include "label_sweep.h"
#include "retain.h"

namespace {

constexpr int RETAIN_WAVES = genphi::RETAIN_THREADS / 64;
constexpr int RETAIN_UNROLL = 4;             // sides a wave has in flight

// Block (blockIdx.x, blockIdx.y): word blockIdx.x of the panel (pair blockIdx.x >> 1, its x or y half) and chunk chunk0 + blockIdx.y.
template <bool TEST_FIRST>
__global__ void __launch_bounds__(genphi::RETAIN_THREADS)
retain_mark_kernel(const ulonglong2 *__restrict__ rows, const int *__restrict__ pro_row, const long long *__restrict__ const_side, int n_pro,
                   long long n_labels, int Pn, int B, long long first_pair, long long S, long long chunk0, int LC, int stride,
                   int *__restrict__ survived, int *__restrict__ both, int *__restrict__ distinct)
{
    extern __shared__ unsigned bitmaps[];                // 64 x stride dwords
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int word = blockIdx.x;
    const long long abs_word = 2 * first_pair + word;
    const u64 cols = column_mask(S, abs_word);
    if (cols == 0) return;                               // (uniform) the last pair's second word holds no column < S
    const bool live_col = (cols >> lane) & 1;
    const long long l0 = (chunk0 + blockIdx.y) * LC;
    const int own = static_cast<int>(min(static_cast<long long>(LC), n_labels - l0));     // the chunk's own labels; a ragged last chunk has fewer
    const int n_dwords = LC / 32 + 1;

    for (int i = threadIdx.x; i < 64 * stride; i += genphi::RETAIN_THREADS) bitmaps[i] = 0u;
    __syncthreads();

    // ---- mark ----
    const u64 *halves = reinterpret_cast<const u64 *>(rows) + (word & 1);
    const long long pair = word >> 1;
    const int n_sides = 2 * n_pro;
    unsigned *mine = bitmaps + lane * stride;
    for (int u0 = wave; u0 < n_sides; u0 += RETAIN_WAVES * RETAIN_UNROLL) {
        unsigned lo[RETAIN_UNROLL], hi[RETAIN_UNROLL];
#pragma unroll
        for (int q = 0; q < RETAIN_UNROLL; ++q) {
            const int u = u0 + q * RETAIN_WAVES;
            u64 w = 0;
            if (u < n_sides && lane < B) {
                const long long e = ((static_cast<long long>(pro_row[u >> 1]) * Pn + pair) * 2 + (u & 1)) * B + lane;
                w = halves[2 * e];
            }
            lo[q] = static_cast<unsigned>(w);
            hi[q] = static_cast<unsigned>(w >> 32);
        }
#pragma unroll
        for (int q = 0; q < RETAIN_UNROLL; ++q) {
            if (u0 + q * RETAIN_WAVES >= n_sides) break;             // (uniform)
            unsigned label = 0;
            for (int b = 0; b < B; ++b) {
                const unsigned wl = __builtin_amdgcn_readlane(lo[q], b), wh = __builtin_amdgcn_readlane(hi[q], b);
                label |= (((lane < 32 ? wl : wh) >> (lane & 31)) & 1u) << b;
            }
            const long long rel = static_cast<long long>(label) - l0;
            if (live_col && rel >= 0 && rel <= LC) {
                unsigned *dst = mine + (rel >> 5);
                const unsigned bit = 1u << (rel & 31);
                if (!TEST_FIRST || !(*static_cast<volatile unsigned *>(dst) & bit)) atomicOr(dst, bit);
            }
        }
    }
    __syncthreads();

    // ---- reduce ----
    const long long col = 64 * abs_word + lane;
    const int own_dwords = (own + 31) / 32;
    int seen = 0;
    for (int d = wave; d < own_dwords; d += RETAIN_WAVES) {
        const unsigned x = mine[d];
        const unsigned next = d + 1 < n_dwords ? mine[d + 1] : 0u;
        const int left = own - 32 * d;                               // the chunk's own labels in this dword and after
        seen += __popc(left >= 32 ? x : x & ((1u << left) - 1u));
        int n_surv = 0, n_both = 0;
        u64 cur = __ballot((x & 1u) != 0) & cols;
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            const u64 nxt = __ballot(((k < 31 ? x >> (k + 1) : next) & 1u) != 0) & cols;
            if (lane == k) {
                n_surv = __popcll(cur);
                n_both = __popcll(cur & nxt);
            }
            cur = nxt;
        }
        const long long l = l0 + 32 * d + lane;
        if (lane < 32 && lane < left) {
            if (n_surv) atomicAdd(survived + l, n_surv);
            if (n_both && l + 1 < n_labels && (const_side[l] >> 1) == (const_side[l + 1] >> 1)) atomicAdd(both + l, n_both);
        }
    }
    if (seen && live_col) atomicAdd(distinct + col, seen);
}

}  // namespace

struct genphi_retain : LabelSweep {          // d_slots: the rows of one panel (n_live x pairs x 2 sides x B planes x 16 bytes)
    genphi::RetainChunks chunks;             // the chunk rule (retain.h)
    bool test_first = false;                 // the mark phase's form
    DevBuf<int> d_survived, d_both, d_distinct;
    DropPanels panels;
    double mark_ms = 0.0, mark_bytes = 0.0;
    genphi_retain() { own(d_survived, d_both, d_distinct); }
};

namespace {

// The panel width, the rows, the results and the lists on the device; GENPHI_ERR_ALLOC before any launch.
int prepare(genphi_retain *h)
{
    const genphi::IdentPlan &pl = h->plan;
    const genphi::RetainSizes z = genphi::retain_sizes(pl, h->S);
    double usable = 0.0;
    if (int rc = h->usable_bytes(usable, h->held_bytes())) return rc;
    const double room = usable - static_cast<double>(z.fixed()) - (64 << 20);
    const double pair_bytes = static_cast<double>(z.panel(1));
    int64_t Pn;
    if (!genphi::drop_panel_fits(Pn, h->S, h->panel_arg, room, pair_bytes))
        return genphi_set_error(GENPHI_ERR_ALLOC, "gen.simuRetention: the counts of " + std::to_string(pl.n_labels) + " founder alleles and " +
                                                      std::to_string(h->S) + " simulations, the lists and " + std::to_string(pl.n_live) + " live rows of " +
                                                      std::to_string(pl.planes) + " planes and " + std::to_string(128 * std::max<int64_t>(Pn, 1)) +
                                                      " simulations do not fit on device " + std::to_string(h->device));
    GENPHI_HIP_TRY(h->d_slots.reserve(z.pair_rows * static_cast<size_t>(Pn)));
    GENPHI_HIP_TRY(h->d_survived.reserve(z.survived / 4));
    GENPHI_HIP_TRY(h->d_both.reserve(z.both / 4));
    GENPHI_HIP_TRY(h->d_distinct.reserve(z.distinct / 4));
    if (int rc = h->upload_lists()) return rc;
    h->panels.set(h->S, Pn);
    return GENPHI_OK;
}

int compute_impl(genphi_retain *h, int32_t device)
{
    if (int rc = h->select(device)) return rc;
    if (int rc = prepare(h)) return rc;
    const genphi::IdentPlan &pl = h->plan;
    const genphi::RetainChunks &ch = h->chunks;
    const int Pn = h->panels.pairs, B = pl.planes, n_pro = static_cast<int>(pl.n_pro);
    const int64_t total = h->panels.total;
    ulonglong2 *rows = h->slots<ulonglong2>();
    const auto mark = h->test_first ? retain_mark_kernel<true> : retain_mark_kernel<false>;
    if (ch.lds_bytes > 32768)
        GENPHI_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(mark), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(ch.lds_bytes)));
    PhaseTimer timer;
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_survived.get(), 0, h->d_survived.bytes(), h->stream));
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_both.get(), 0, h->d_both.bytes(), h->stream));
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_distinct.get(), 0, h->d_distinct.bytes(), h->stream));
    double sweep_ms = 0.0, mark_ms = 0.0;
    int64_t launches = 0;
    for (int64_t p0 = 0; p0 < total; p0 += Pn) {
        const int Pc = static_cast<int>(std::min<int64_t>(Pn, total - p0));
        if (int rc = timer.begin(h->stream)) return rc;
        if (int rc = label_sweep_panel(h, Pc, static_cast<unsigned>(p0))) return rc;
        if (int rc = timer.middle(h->stream)) return rc;
        for (int64_t c0 = 0; c0 < ch.chunks; c0 += 65535) {          // (a grid's y extent)
            const dim3 grid(static_cast<unsigned>(2 * Pc), static_cast<unsigned>(std::min<int64_t>(65535, ch.chunks - c0)));
            mark<<<grid, genphi::RETAIN_THREADS, ch.lds_bytes, h->stream>>>(rows, h->d_pro_row.get(), h->d_const_side.get(), n_pro, pl.n_labels, Pn, B, p0, h->S, c0,
                                                                           static_cast<int>(ch.chunk_labels), ch.stride, h->d_survived.get(), h->d_both.get(),
                                                                           h->d_distinct.get());
            GENPHI_HIP_TRY(hipGetLastError());
            ++launches;
        }
        if (int rc = timer.end(h->stream)) return rc;
        if (int rc = timer.add(sweep_ms, mark_ms)) return rc;
        launches += pl.n_levels;
    }
    GENPHI_HIP_TRY(hipStreamSynchronize(h->stream));
    // the sweep's bytes are ident's: per side with a known parent two runs of B planes read and one written, 16 bytes per plane and pair
    const double known_sides = 2.0 * static_cast<double>(pl.n_live) - static_cast<double>(pl.n_labels);
    h->sweep_ms = sweep_ms;
    h->mark_ms = mark_ms;
    h->alg_bytes = 3.0 * 16.0 * B * known_sides * static_cast<double>(total);
    h->mark_bytes = 2.0 * n_pro * B * 16.0 * static_cast<double>(total) * static_cast<double>(ch.chunks);
    h->n_launches = launches;
    h->computed = true;
    return GENPHI_OK;
}

}  // namespace

extern "C" {

int genphi_retain_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro, const int64_t *pro_ids,
                         int64_t simul_no, uint64_t seed, int32_t panel_cols, int32_t chunk_labels, int32_t flags, genphi_retain **out)
{
    if (out) *out = nullptr;
    if (out && (flags & ~(GENPHI_RETAIN_FLAG_PLAIN_OR | GENPHI_RETAIN_FLAG_TEST_FIRST))) return genphi_set_error(GENPHI_ERR_ARG, "genphi_retain_create: unknown flag");
    if (out && flags == (GENPHI_RETAIN_FLAG_PLAIN_OR | GENPHI_RETAIN_FLAG_TEST_FIRST))
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_retain_create: GENPHI_RETAIN_FLAG_PLAIN_OR and GENPHI_RETAIN_FLAG_TEST_FIRST exclude each other");
    if (int rc = check_create_args("genphi_retain_create", n_ind, ind, father, mother, n_pro, pro_ids, 0, nullptr, out, 0)) return rc;
    if (n_pro == 0) return genphi_set_error(GENPHI_ERR_ARG, "gen.simuRetention: no probands");
    if (simul_no < 1 || simul_no > GENPHI_SIMU_MAX_SIMULATIONS)
        return genphi_set_error(GENPHI_ERR_ARG, "gen.simuRetention: simulNo = " + std::to_string(simul_no) + " is outside 1 .. 2^24");
    if (panel_cols < 0) return genphi_set_error(GENPHI_ERR_ARG, "genphi_retain_create: panel_cols is 0 (the default rule) or positive");
    if (chunk_labels < 0) return genphi_set_error(GENPHI_ERR_ARG, "genphi_retain_create: chunk_labels is 0 (the default rule) or positive");
    return create_entry(out, "gen.simuRetention", [&](genphi_retain *h) {
        h->S = simul_no;
        h->seed = seed;
        h->test_first = flags ? (flags & GENPHI_RETAIN_FLAG_TEST_FIRST) != 0 : genphi::RETAIN_DEFAULT_TEST_FIRST != 0;
        h->panel_arg = panel_cols;
        std::string err;
        if (const int rc = genphi::plan_ident(h->plan, n_ind, ind, father, mother, n_pro, pro_ids, err)) return genphi_set_error(rc, err);
        h->chunks = genphi::retain_chunks(h->plan.n_labels, chunk_labels);
        h->panels.set(simul_no, genphi::drop_panel_pairs(simul_no, panel_cols));                // (compute may narrow the default to what fits)
        return GENPHI_OK;
    });
}

int genphi_retain_levels(const genphi_retain *h, int64_t *n_live, int32_t *levels, int64_t *rows_per_level)
{
    return drop_levels(h, "genphi_retain_levels", n_live, levels, rows_per_level);
}

int genphi_retain_alleles(const genphi_retain *h, int64_t *n_labels, int32_t *planes, int64_t *ids, int32_t *sides)
{
    return label_alleles(h, "genphi_retain_alleles", n_labels, planes, ids, sides);
}

int genphi_retain_compute(genphi_retain *h, int32_t device) { return compute_entry(h, device, "genphi_retain_compute", "gen.simuRetention", compute_impl); }

int genphi_retain_survived_to_host(genphi_retain *h, int32_t *out)
{
    return result_to_host(h, out, &genphi_retain::d_survived, "genphi_retain_survived_to_host", "gen.simuRetention");
}

int genphi_retain_both_to_host(genphi_retain *h, int32_t *out)
{
    return result_to_host(h, out, &genphi_retain::d_both, "genphi_retain_both_to_host", "gen.simuRetention");
}

int genphi_retain_distinct_to_host(genphi_retain *h, int32_t *out)
{
    return result_to_host(h, out, &genphi_retain::d_distinct, "genphi_retain_distinct_to_host", "gen.simuRetention");
}

int genphi_retain_stats(const genphi_retain *h, double *sweep_ms, double *mark_ms, double *algorithmic_bytes, double *mark_bytes, int32_t *levels,
                        int32_t *panel_cols, int64_t *panels, int32_t *planes, int32_t *chunk_labels, int64_t *chunks, int32_t *lds_bytes,
                        int32_t *lanes_per_row)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_retain_stats: NULL handle");
    h->stats(sweep_ms, algorithmic_bytes, nullptr);
    put(mark_ms, h->mark_ms);
    put(mark_bytes, h->mark_bytes);
    put(levels, h->plan.n_levels);
    put(panel_cols, 128 * h->panels.pairs);
    put(panels, h->panels.n_panels);
    put(planes, h->plan.planes);
    put(chunk_labels, h->chunks.chunk_labels);
    put(chunks, h->chunks.chunks);
    put(lds_bytes, h->chunks.lds_bytes);
    put(lanes_per_row, h->panels.lanes_per_row);
    return GENPHI_OK;
}

void genphi_retain_destroy(genphi_retain *h) { destroy_entry(h); }

}  // extern "C"
