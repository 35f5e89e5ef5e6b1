// unique.hip -- gen.simuUniqueness: for every proband, with how many members of the population it shares each founder allele it
// carries, by gene dropping (include/genphi.h, genphi_unique_*).  The label sweep is the shared one (label_sweep.h: the base of the
// handle, the init kernel and the step kernel, on ident's columns: row r, pair j, side s, plane b at ((r * Pn + j) * 2 + s) * B + b,
// 16-byte elements); the plan is ident.h's on the probands followed by the others.  Only the reduction is new, and it is the hot path:
//   count   one launch per panel after the last level, grid (words of the panel, label chunks), 1,024 threads.  A workgroup owns the
//           64 simulations of one word and the labels [l0, l0 + LC) of one chunk (unique.h: unique_chunks).  It holds 64 tables in LDS,
//           one per simulation, of 16-bit counters, two labels to a dword: label t of the chunk in half t & 1 of dword t >> 1.  Lane s
//           of every wave is simulation s: the lanes of a wave never meet in one dword, only waves do, and those are resolved by
//           32-bit LDS atomics (n_pop <= 65,535: no add carries from one half into the other, unique.h).  The tables lie
//           stride = ceil(LC / 2) | 1 dwords apart: for one dword the 64 lanes fall on 64 different banks.
//           1. zero the tables.
//           2. count: wave v takes the individuals i = v, v + 16, .. of the population (unique.h: the distinct probands, then the
//              distinct others), read in place (there is no gather).  The decode is carry.hip's: lane b < B loads its word's half of
//              plane b of side 0 and lane 32 + b that of side 1, one 8-byte load per lane and individual; the two labels of lane s
//              are then bit s of the 2 B words, which reach every lane as wave-uniform values (readlane).  Four individuals are loaded
//              before the first is decoded.  A column < S adds 1 to the field of a when a lies in the chunk, and to that of b when
//              b != a and b lies in the chunk: c1.
//           3. a barrier.
//           4. attribute: the waves walk the n probands again, decoded the same way.  A side whose label lies in the chunk reads the
//              field m of its own table and adds 1 at alleles[i K + min(m, K) - 1], once when a = b, and then also 1 at the same cell
//              of autozygous.  The lanes of a wave that meet in one of the first UNIQUE_AGG columns are counted by a ballot and
//              added by one lane (hist.hip's aggregation); the rest add their own 1.  Measured against one atomic per lane
//              (DESIGN.md 31): 2.7 times faster with 140 probands, whose few cells every wave meets in, 3 % faster with 2,000 and
//              3 % slower with 10,000.  GENPHI_UNIQUE_ATTRIBUTE (an environment hook, planner.h) picks the form for that A/B:
//              1 = one atomic per lane, 2 = aggregated.
// Nothing couples neighbouring labels: no halo.  Everything is integer; the only atomics on global memory are integer adds: the same
// bytes on every run, with any panel, chunk and form.
#include <hip/hip_runtime.h>

#include "label_sweep.h"
#include "unique.h"

namespace {

constexpr int UNIQUE_WAVES = genphi::UNIQUE_THREADS / 64;
constexpr int UNIQUE_UNROLL = 4;             // individuals a wave has in flight
constexpr int UNIQUE_AGG = 4;                // the columns the aggregating form counts by ballot

// Wave `wave` of UNIQUE_WAVES walks the individuals i = wave, wave + 16, .. < n of ind_row, four in flight, and calls f(i, a, b) with
// the two labels of lane s = simulation s of the word.  Every lane of the wave calls f the same number of times: f may ballot.
template <class F>
__device__ __forceinline__ void walk_sides(const u64 *__restrict__ halves, const int *__restrict__ ind_row, int n, int Pn, int B, long long pair, int wave,
                                           int lane, F f)
{
    const int side = lane >> 5, plane = lane & 31;
    for (int i0 = wave; i0 < n; i0 += UNIQUE_WAVES * UNIQUE_UNROLL) {
        unsigned lo[UNIQUE_UNROLL], hi[UNIQUE_UNROLL];
#pragma unroll
        for (int q = 0; q < UNIQUE_UNROLL; ++q) {
            const int i = i0 + q * UNIQUE_WAVES;
            u64 w = 0;
            if (i < n && plane < B) {
                const long long e = ((static_cast<long long>(ind_row[i]) * Pn + pair) * 2 + side) * B + plane;
                w = halves[2 * e];
            }
            lo[q] = static_cast<unsigned>(w);
            hi[q] = static_cast<unsigned>(w >> 32);
        }
#pragma unroll
        for (int q = 0; q < UNIQUE_UNROLL; ++q) {
            const int i = i0 + q * UNIQUE_WAVES;
            if (i >= n) break;                                           // (uniform)
            unsigned a = 0, b = 0;
            for (int p = 0; p < B; ++p) {
                const unsigned al = __builtin_amdgcn_readlane(lo[q], p), ah = __builtin_amdgcn_readlane(hi[q], p);
                const unsigned bl = __builtin_amdgcn_readlane(lo[q], 32 + p), bh = __builtin_amdgcn_readlane(hi[q], 32 + p);
                a |= (((lane < 32 ? al : ah) >> (lane & 31)) & 1u) << p;
                b |= (((lane < 32 ? bl : bh) >> (lane & 31)) & 1u) << p;
            }
            f(i, a, b);
        }
    }
}

// One more in row[col] for every lane with `take`; all 64 lanes of the wave call this together.  AGG: the lanes that meet in one of
// the columns 0 .. UNIQUE_AGG - 1 are counted by a ballot and added by the first of them.
template <bool AGG>
__device__ __forceinline__ void bump(int *row, int col, bool take, int lane)
{
    if (AGG) {
        if (!__ballot(take)) return;                                     // (uniform) no side of this wave lies in the chunk
#pragma unroll
        for (int c = 0; c < UNIQUE_AGG; ++c) {
            const u64 same = __ballot(take && col == c);
            if (same && lane == __ffsll(static_cast<long long>(same)) - 1) atomicAdd(row + c, __popcll(same));
        }
        take = take && col >= UNIQUE_AGG;
    }
    if (take) atomicAdd(row + col, 1);
}

// Block (blockIdx.x, blockIdx.y): word blockIdx.x of the panel (pair blockIdx.x >> 1, its x or y half) and chunk chunk0 + blockIdx.y.
template <bool AGG>
__global__ void __launch_bounds__(genphi::UNIQUE_THREADS)
unique_count_kernel(const ulonglong2 *__restrict__ rows, const int *__restrict__ ind_row, int n_pro, int n_pop, long long n_labels, int Pn, int B,
                    long long first_pair, long long S, long long chunk0, int LC, int stride, int K, int *__restrict__ alleles, int *__restrict__ autozygous)
{
    extern __shared__ unsigned tables[];                 // 64 x stride dwords
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int word = blockIdx.x;
    const long long abs_word = 2 * first_pair + word;
    const u64 cols = column_mask(S, abs_word);
    if (cols == 0) return;                               // (uniform) the last pair's second word holds no column < S
    const bool live_col = (cols >> lane) & 1;
    const long long l0 = (chunk0 + blockIdx.y) * LC;
    const int own = static_cast<int>(min(static_cast<long long>(LC), n_labels - l0));     // a ragged last chunk has fewer labels

    for (int i = threadIdx.x; i < 64 * stride; i += genphi::UNIQUE_THREADS) tables[i] = 0u;
    __syncthreads();

    const u64 *halves = reinterpret_cast<const u64 *>(rows) + (word & 1);
    const long long pair = word >> 1;
    unsigned *mine = tables + lane * stride;

    // ---- count: c1 over the population ----
    walk_sides(halves, ind_row, n_pop, Pn, B, pair, wave, lane, [&](int, unsigned a, unsigned b) {
        const long long ra = static_cast<long long>(a) - l0, rb = static_cast<long long>(b) - l0;
        const bool in_a = live_col && ra >= 0 && ra < own, in_b = live_col && b != a && rb >= 0 && rb < own;
        if (in_a) atomicAdd(mine + (ra >> 1), 1u << (16 * (ra & 1)));
        if (in_b) atomicAdd(mine + (rb >> 1), 1u << (16 * (rb & 1)));
    });
    __syncthreads();

    // ---- attribute: every proband's sides to the column of their share ----
    const unsigned top = static_cast<unsigned>(K);
    walk_sides(halves, ind_row, n_pro, Pn, B, pair, wave, lane, [&](int i, unsigned a, unsigned b) {
        const long long ra = static_cast<long long>(a) - l0, rb = static_cast<long long>(b) - l0;
        const bool in_a = live_col && ra >= 0 && ra < own, in_b = live_col && b != a && rb >= 0 && rb < own;
        // the proband itself was counted: m >= 1 (the max keeps the column inside the row whatever the table holds)
        const unsigned ma = in_a ? (mine[ra >> 1] >> (16 * (ra & 1))) & 0xFFFFu : 1u, mb = in_b ? (mine[rb >> 1] >> (16 * (rb & 1))) & 0xFFFFu : 1u;
        const int col_a = static_cast<int>(min(max(ma, 1u), top)) - 1, col_b = static_cast<int>(min(max(mb, 1u), top)) - 1;
        const long long at = static_cast<long long>(i) * K;
        bump<AGG>(alleles + at, col_a, in_a, lane);
        bump<AGG>(alleles + at, col_b, in_b, lane);
        bump<AGG>(autozygous + at, col_a, in_a && a == b, lane);
    });
}

}  // namespace

struct genphi_unique : LabelSweep {          // d_slots: the rows of one panel (n_live x pairs x 2 sides x B planes x 16 bytes)
    genphi::UniqueLists lists;               // the population as rows (unique.h)
    genphi::UniqueChunks chunks;             // the chunk rule (unique.h)
    int64_t K = 0;                           // the columns of alleles / autozygous
    bool aggregate = true;                   // the form of the attribute phase
    DevBuf<int> d_ind_row, d_alleles, d_autozygous;
    DropPanels panels;
    double count_ms = 0.0, count_bytes = 0.0;
    genphi_unique() { own(d_ind_row, d_alleles, d_autozygous); }
};

namespace {

// The panel width, the rows, the results and the lists on the device; GENPHI_ERR_ALLOC before any launch.
int prepare(genphi_unique *h)
{
    const genphi::IdentPlan &pl = h->plan;
    const genphi::UniqueSizes z = genphi::unique_sizes(pl, h->lists, h->K);
    double usable = 0.0;
    if (int rc = h->usable_bytes(usable, h->held_bytes())) return rc;
    const double room = usable - static_cast<double>(z.fixed()) - (64 << 20);
    const double pair_bytes = static_cast<double>(z.panel(1));
    int64_t Pn;
    if (!genphi::drop_panel_fits(Pn, h->S, h->panel_arg, room, pair_bytes))
        return genphi_set_error(GENPHI_ERR_ALLOC, "gen.simuUniqueness: the shares of " + std::to_string(h->lists.n_pro) + " probands in " + std::to_string(h->K) +
                                                      " columns, the lists and " + std::to_string(pl.n_live) + " live rows of " + std::to_string(pl.planes) +
                                                      " planes and " + std::to_string(128 * std::max<int64_t>(Pn, 1)) + " simulations do not fit on device " +
                                                      std::to_string(h->device));
    GENPHI_HIP_TRY(h->d_slots.reserve(z.pair_rows * static_cast<size_t>(Pn)));
    GENPHI_HIP_TRY(h->d_alleles.reserve(z.alleles / 4));
    GENPHI_HIP_TRY(h->d_autozygous.reserve(z.autozygous / 4));
    if (int rc = h->upload_lists()) return rc;
    if (int rc = h->upload(h->d_ind_row, h->lists.rows)) return rc;
    h->panels.set(h->S, Pn);
    return GENPHI_OK;
}

template <bool AGG>
int count_panel(genphi_unique *h, int Pc, int64_t p0, int64_t &launches)
{
    const genphi::IdentPlan &pl = h->plan;
    const genphi::UniqueChunks &ch = h->chunks;
    if (ch.lds_bytes > 32768)
        GENPHI_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(unique_count_kernel<AGG>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           static_cast<int>(ch.lds_bytes)));
    for (int64_t c0 = 0; c0 < ch.chunks; c0 += 65535) {              // (a grid's y extent)
        const dim3 grid(static_cast<unsigned>(2 * Pc), static_cast<unsigned>(std::min<int64_t>(65535, ch.chunks - c0)));
        unique_count_kernel<AGG><<<grid, genphi::UNIQUE_THREADS, ch.lds_bytes, h->stream>>>(
            h->slots<ulonglong2>(), h->d_ind_row.get(), static_cast<int>(h->lists.n_pro), static_cast<int>(h->lists.n_pop()), pl.n_labels, h->panels.pairs, pl.planes,
            p0, h->S, c0, static_cast<int>(ch.chunk_labels), ch.stride, static_cast<int>(h->K), h->d_alleles.get(), h->d_autozygous.get());
        GENPHI_HIP_TRY(hipGetLastError());
        ++launches;
    }
    return GENPHI_OK;
}

int compute_impl(genphi_unique *h, int32_t device)
{
    if (int rc = h->select(device)) return rc;
    if (int rc = prepare(h)) return rc;
    const genphi::IdentPlan &pl = h->plan;
    const int Pn = h->panels.pairs, B = pl.planes;
    const int64_t total = h->panels.total;
    PhaseTimer timer;
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_alleles.get(), 0, h->d_alleles.bytes(), h->stream));
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_autozygous.get(), 0, h->d_autozygous.bytes(), h->stream));
    double sweep_ms = 0.0, count_ms = 0.0;
    int64_t launches = 0;
    for (int64_t p0 = 0; p0 < total; p0 += Pn) {
        const int Pc = static_cast<int>(std::min<int64_t>(Pn, total - p0));
        if (int rc = timer.begin(h->stream)) return rc;
        if (int rc = label_sweep_panel(h, Pc, static_cast<unsigned>(p0))) return rc;
        if (int rc = timer.middle(h->stream)) return rc;
        if (int rc = h->aggregate ? count_panel<true>(h, Pc, p0, launches) : count_panel<false>(h, Pc, p0, launches)) return rc;
        if (int rc = timer.end(h->stream)) return rc;
        if (int rc = timer.add(sweep_ms, count_ms)) return rc;
        launches += pl.n_levels;
    }
    GENPHI_HIP_TRY(hipStreamSynchronize(h->stream));
    // the sweep's bytes are ident's: per side with a known parent two runs of B planes read and one written, 16 bytes per plane and pair
    const double known_sides = 2.0 * static_cast<double>(pl.n_live) - static_cast<double>(pl.n_labels);
    h->sweep_ms = sweep_ms;
    h->count_ms = count_ms;
    h->alg_bytes = 3.0 * 16.0 * B * known_sides * static_cast<double>(total);
    // a chunk reads the planes of the population once and those of the probands once more
    h->count_bytes = 2.0 * static_cast<double>(h->lists.n_pop() + h->lists.n_pro) * B * 16.0 * static_cast<double>(total) * static_cast<double>(h->chunks.chunks);
    h->n_launches = launches;
    h->computed = true;
    return GENPHI_OK;
}

}  // namespace

extern "C" {

int genphi_unique_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro, const int64_t *pro_ids,
                         int64_t n_others, const int64_t *other_ids, int64_t simul_no, uint64_t seed, int32_t panel_cols, int32_t chunk_labels,
                         int32_t max_share, genphi_unique **out)
{
    if (out) *out = nullptr;
    if (int rc = check_create_args("genphi_unique_create", n_ind, ind, father, mother, n_pro, pro_ids, n_others, other_ids, out, INT32_MAX)) return rc;
    if (n_pro == 0) return genphi_set_error(GENPHI_ERR_ARG, "gen.simuUniqueness: no probands");
    if (n_pro + n_others >= INT32_MAX) return genphi_set_error(GENPHI_ERR_ARG, "genphi_unique_create: more than 2^31 - 2 probands and others");
    if (simul_no < 1 || simul_no > GENPHI_SIMU_MAX_SIMULATIONS)
        return genphi_set_error(GENPHI_ERR_ARG, "gen.simuUniqueness: simulNo = " + std::to_string(simul_no) + " is outside 1 .. 2^24");
    if (panel_cols < 0) return genphi_set_error(GENPHI_ERR_ARG, "genphi_unique_create: panel_cols is 0 (the default rule) or positive");
    if (chunk_labels < 0) return genphi_set_error(GENPHI_ERR_ARG, "genphi_unique_create: chunk_labels is 0 (the default rule) or positive");
    if (max_share < 0) return genphi_set_error(GENPHI_ERR_ARG, "genphi_unique_create: max_share is 0 (every share has its column) or positive");
    return create_entry(out, "gen.simuUniqueness", [&](genphi_unique *h) {
        h->S = simul_no;
        h->seed = seed;
        h->panel_arg = panel_cols;
        if (const int32_t form = hook_count("GENPHI_UNIQUE_ATTRIBUTE")) h->aggregate = form != 1;
        std::vector<int64_t> listed(pro_ids, pro_ids + n_pro);
        listed.insert(listed.end(), other_ids, other_ids + n_others);
        std::string err;
        if (const int rc = genphi::plan_ident(h->plan, n_ind, ind, father, mother, static_cast<int64_t>(listed.size()), listed.data(), err))
            return genphi_set_error(rc, err);
        genphi::unique_lists(h->lists, h->plan, n_pro);
        h->K = genphi::unique_columns(h->lists.n_pop(), max_share);
        const std::string limit = genphi::unique_limits(h->lists.n_pro, h->lists.n_pop(), h->K);
        if (!limit.empty()) return genphi_set_error(GENPHI_ERR_ARG, "gen.simuUniqueness: " + limit);
        h->chunks = genphi::unique_chunks(h->plan.n_labels, chunk_labels);
        h->panels.set(simul_no, genphi::drop_panel_pairs(simul_no, panel_cols));                // (compute may narrow the default to what fits)
        return GENPHI_OK;
    });
}

int genphi_unique_levels(const genphi_unique *h, int64_t *n_live, int32_t *levels, int64_t *rows_per_level)
{
    return drop_levels(h, "genphi_unique_levels", n_live, levels, rows_per_level);
}

int genphi_unique_alleles(const genphi_unique *h, int64_t *n_labels, int32_t *planes, int64_t *ids, int32_t *sides)
{
    return label_alleles(h, "genphi_unique_alleles", n_labels, planes, ids, sides);
}

int genphi_unique_probands(const genphi_unique *h, int64_t *n, int64_t *ids)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_unique_probands: NULL handle");
    put(n, h->lists.n_pro);
    if (ids)
        for (int64_t i = 0; i < h->lists.n_pro; ++i) ids[i] = h->plan.row_id[h->lists.rows[i]];
    return GENPHI_OK;
}

int genphi_unique_compute(genphi_unique *h, int32_t device) { return compute_entry(h, device, "genphi_unique_compute", "gen.simuUniqueness", compute_impl); }

int genphi_unique_alleles_to_host(genphi_unique *h, int32_t *out)
{
    return result_to_host(h, out, &genphi_unique::d_alleles, "genphi_unique_alleles_to_host", "gen.simuUniqueness");
}

int genphi_unique_autozygous_to_host(genphi_unique *h, int32_t *out)
{
    return result_to_host(h, out, &genphi_unique::d_autozygous, "genphi_unique_autozygous_to_host", "gen.simuUniqueness");
}

int genphi_unique_stats(const genphi_unique *h, double *sweep_ms, double *count_ms, double *algorithmic_bytes, double *count_bytes, int32_t *levels,
                        int32_t *panel_cols, int64_t *panels, int32_t *planes, int32_t *chunk_labels, int64_t *chunks, int32_t *lds_bytes, int32_t *columns,
                        int32_t *n, int32_t *n_pop)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_unique_stats: NULL handle");
    h->stats(sweep_ms, algorithmic_bytes, nullptr);
    put(count_ms, h->count_ms);
    put(count_bytes, h->count_bytes);
    put(levels, h->plan.n_levels);
    put(panel_cols, 128 * h->panels.pairs);
    put(panels, h->panels.n_panels);
    put(planes, h->plan.planes);
    put(chunk_labels, h->chunks.chunk_labels);
    put(chunks, h->chunks.chunks);
    put(lds_bytes, h->chunks.lds_bytes);
    put(columns, h->K);
    put(n, h->lists.n_pro);
    put(n_pop, h->lists.n_pop());
    return GENPHI_OK;
}

void genphi_unique_destroy(genphi_unique *h) { destroy_entry(h); }

}  // extern "C"
