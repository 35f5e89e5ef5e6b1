// carry.hip -- gen.simuCarriers: how many of the listed cases carry every founder allele, by gene dropping (include/genphi.h,
// genphi_carry_*).  The label sweep is the shared one (label_sweep.h: the base of the handle, the init kernel and the step kernel, on
// ident's columns: row r, pair j, side s, plane b at ((r * Pn + j) * 2 + s) * B + b, 16-byte elements); the plan is ident.h's on the
// cases followed by the controls.  Only the reduction is new, and it is the hot path:
//   count   one launch per panel after the last level, grid (words of the panel, label chunks), 1,024 threads.  A workgroup owns the
//           64 simulations of one word and the labels [l0, l0 + LC) of one chunk (carry.h: carry_chunks).  It holds 64 tables in LDS,
//           one per simulation, of LC counter dwords: c1 in bits 0-15, c2 in bits 16-30, x in bit 31.  Lane s of every wave is
//           simulation s: the lanes of a wave never meet in one dword, only waves do, and those are resolved by 32-bit LDS atomics.
//           The tables lie stride = LC | 1 dwords apart: for one label the 64 lanes fall on 64 different banks.
//           1. zero the tables.
//           2. count: wave v takes the individuals i = v, v + 16, .. of the row list (carry.h: the distinct cases, then the distinct
//              controls), read in place (there is no gather).  Lane b < B loads its word's half of plane b of side 0 and lane
//              32 + b that of side 1, one 8-byte load per lane and individual; the two labels of lane s are then bit s of the 2 B
//              words, which reach every lane as wave-uniform values (readlane).  Four individuals are loaded before the first is
//              decoded.  A column < S adds into the dwords of its labels that lie in the chunk: a case 1 at a and 1 at b, or 0x10001
//              at a when a = b; a control sets bit 31.  At most 32,767 cases: no field carries into the next.
//           3. reduce, after a barrier, the chunk's labels dealt to the waves: lane s reads the dword of its own table.  x set: the
//              wave's ballot, masked to the columns < S, goes into excluded[l] as one atomicAdd.  Otherwise a lane with c1 >= 1 adds
//              1 at carriers[l W + min(c1, W - 1)], and likewise for c2 and homozygotes.  Column 0 is never written.
// Nothing couples neighbouring labels: no halo.  Everything is integer; the only atomics on global memory are integer adds: the same
// bytes on every run, with any panel and chunk.
#include <hip/hip_runtime.h>

#include "carry.h"
#include "label_sweep.h"

namespace {

constexpr int CARRY_WAVES = genphi::CARRY_THREADS / 64;
constexpr int CARRY_UNROLL = 4;              // individuals a wave has in flight

// Block (blockIdx.x, blockIdx.y): word blockIdx.x of the panel (pair blockIdx.x >> 1, its x or y half) and chunk chunk0 + blockIdx.y.
__global__ void __launch_bounds__(genphi::CARRY_THREADS)
carry_count_kernel(const ulonglong2 *__restrict__ rows, const int *__restrict__ ind_row, int n_cases, int n_ind, long long n_labels, int Pn, int B,
                   long long first_pair, long long S, long long chunk0, int LC, int stride, int W, int *__restrict__ excluded,
                   int *__restrict__ carriers, int *__restrict__ homozygotes)
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

    for (int i = threadIdx.x; i < 64 * stride; i += genphi::CARRY_THREADS) tables[i] = 0u;
    __syncthreads();

    // ---- count ----
    const u64 *halves = reinterpret_cast<const u64 *>(rows) + (word & 1);
    const long long pair = word >> 1;
    const int side = lane >> 5, plane = lane & 31;
    unsigned *mine = tables + lane * stride;
    for (int i0 = wave; i0 < n_ind; i0 += CARRY_WAVES * CARRY_UNROLL) {
        unsigned lo[CARRY_UNROLL], hi[CARRY_UNROLL];
#pragma unroll
        for (int q = 0; q < CARRY_UNROLL; ++q) {
            const int i = i0 + q * CARRY_WAVES;
            u64 w = 0;
            if (i < n_ind && plane < B) {
                const long long e = ((static_cast<long long>(ind_row[i]) * Pn + pair) * 2 + side) * B + plane;
                w = halves[2 * e];
            }
            lo[q] = static_cast<unsigned>(w);
            hi[q] = static_cast<unsigned>(w >> 32);
        }
#pragma unroll
        for (int q = 0; q < CARRY_UNROLL; ++q) {
            const int i = i0 + q * CARRY_WAVES;
            if (i >= n_ind) break;                                       // (uniform)
            unsigned a = 0, b = 0;
            for (int p = 0; p < B; ++p) {
                const unsigned al = __builtin_amdgcn_readlane(lo[q], p), ah = __builtin_amdgcn_readlane(hi[q], p);
                const unsigned bl = __builtin_amdgcn_readlane(lo[q], 32 + p), bh = __builtin_amdgcn_readlane(hi[q], 32 + p);
                a |= (((lane < 32 ? al : ah) >> (lane & 31)) & 1u) << p;
                b |= (((lane < 32 ? bl : bh) >> (lane & 31)) & 1u) << p;
            }
            const long long ra = static_cast<long long>(a) - l0, rb = static_cast<long long>(b) - l0;
            const bool in_a = live_col && ra >= 0 && ra < own, in_b = live_col && b != a && rb >= 0 && rb < own;
            if (i < n_cases) {                                           // (uniform) a case
                if (in_a) atomicAdd(mine + ra, a == b ? 0x10001u : 1u);
                if (in_b) atomicAdd(mine + rb, 1u);
            } else {                                                     // a control
                if (in_a) atomicOr(mine + ra, 0x80000000u);
                if (in_b) atomicOr(mine + rb, 0x80000000u);
            }
        }
    }
    __syncthreads();

    // ---- reduce ----
    const unsigned last = static_cast<unsigned>(W - 1);
    for (int t = wave; t < own; t += CARRY_WAVES) {
        const unsigned v = live_col ? mine[t] : 0u;
        const long long l = l0 + t;
        const u64 out = __ballot(v >> 31);
        if (out && lane == 0) atomicAdd(excluded + l, __popcll(out));
        if (v && !(v >> 31)) {
            const unsigned c1 = v & 0xFFFFu, c2 = (v >> 16) & 0x7FFFu;
            atomicAdd(carriers + (l * W + min(c1, last)), 1);
            if (c2) atomicAdd(homozygotes + (l * W + min(c2, last)), 1);
        }
    }
}

}  // namespace

struct genphi_carry : LabelSweep {           // d_slots: the rows of one panel (n_live x pairs x 2 sides x B planes x 16 bytes)
    genphi::CarryLists lists;                // the two sets of rows (carry.h)
    genphi::CarryChunks chunks;              // the chunk rule (carry.h)
    int64_t W = 0;                           // the columns of carriers / homozygotes
    DevBuf<int> d_ind_row, d_excluded, d_carriers, d_homozygotes;
    DropPanels panels;
    double count_ms = 0.0, count_bytes = 0.0;
    genphi_carry() { own(d_ind_row, d_excluded, d_carriers, d_homozygotes); }
};

namespace {

// The panel width, the rows, the results and the lists on the device; GENPHI_ERR_ALLOC before any launch.
int prepare(genphi_carry *h)
{
    const genphi::IdentPlan &pl = h->plan;
    const genphi::CarrySizes z = genphi::carry_sizes(pl, h->lists, h->W);
    double usable = 0.0;
    if (int rc = h->usable_bytes(usable, h->held_bytes())) return rc;
    const double room = usable - static_cast<double>(z.fixed()) - (64 << 20);
    const double pair_bytes = static_cast<double>(z.panel(1));
    int64_t Pn;
    if (!genphi::drop_panel_fits(Pn, h->S, h->panel_arg, room, pair_bytes))
        return genphi_set_error(GENPHI_ERR_ALLOC, "gen.simuCarriers: the counts of " + std::to_string(pl.n_labels) + " founder alleles in " + std::to_string(h->W) +
                                                      " columns, the lists and " + std::to_string(pl.n_live) + " live rows of " + std::to_string(pl.planes) +
                                                      " planes and " + std::to_string(128 * std::max<int64_t>(Pn, 1)) + " simulations do not fit on device " +
                                                      std::to_string(h->device));
    GENPHI_HIP_TRY(h->d_slots.reserve(z.pair_rows * static_cast<size_t>(Pn)));
    GENPHI_HIP_TRY(h->d_excluded.reserve(z.excluded / 4));
    GENPHI_HIP_TRY(h->d_carriers.reserve(z.carriers / 4));
    GENPHI_HIP_TRY(h->d_homozygotes.reserve(z.homozygotes / 4));
    if (int rc = h->upload_lists()) return rc;
    if (int rc = h->upload(h->d_ind_row, h->lists.rows)) return rc;
    h->panels.set(h->S, Pn);
    return GENPHI_OK;
}

int compute_impl(genphi_carry *h, int32_t device)
{
    if (int rc = h->select(device)) return rc;
    if (int rc = prepare(h)) return rc;
    const genphi::IdentPlan &pl = h->plan;
    const genphi::CarryChunks &ch = h->chunks;
    const int Pn = h->panels.pairs, B = pl.planes, n_cases = static_cast<int>(h->lists.n_cases), n_ind = static_cast<int>(h->lists.rows.size());
    const int64_t total = h->panels.total;
    ulonglong2 *rows = h->slots<ulonglong2>();
    if (ch.lds_bytes > 32768)
        GENPHI_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(carry_count_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           static_cast<int>(ch.lds_bytes)));
    PhaseTimer timer;
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_excluded.get(), 0, h->d_excluded.bytes(), h->stream));
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_carriers.get(), 0, h->d_carriers.bytes(), h->stream));
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_homozygotes.get(), 0, h->d_homozygotes.bytes(), h->stream));
    double sweep_ms = 0.0, count_ms = 0.0;
    int64_t launches = 0;
    for (int64_t p0 = 0; p0 < total; p0 += Pn) {
        const int Pc = static_cast<int>(std::min<int64_t>(Pn, total - p0));
        if (int rc = timer.begin(h->stream)) return rc;
        if (int rc = label_sweep_panel(h, Pc, static_cast<unsigned>(p0))) return rc;
        if (int rc = timer.middle(h->stream)) return rc;
        for (int64_t c0 = 0; c0 < ch.chunks; c0 += 65535) {          // (a grid's y extent)
            const dim3 grid(static_cast<unsigned>(2 * Pc), static_cast<unsigned>(std::min<int64_t>(65535, ch.chunks - c0)));
            carry_count_kernel<<<grid, genphi::CARRY_THREADS, ch.lds_bytes, h->stream>>>(rows, h->d_ind_row.get(), n_cases, n_ind, pl.n_labels, Pn, B, p0, h->S, c0,
                                                                                         static_cast<int>(ch.chunk_labels), ch.stride, static_cast<int>(h->W),
                                                                                         h->d_excluded.get(), h->d_carriers.get(), h->d_homozygotes.get());
            GENPHI_HIP_TRY(hipGetLastError());
            ++launches;
        }
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
    h->count_bytes = 2.0 * n_ind * B * 16.0 * static_cast<double>(total) * static_cast<double>(ch.chunks);
    h->n_launches = launches;
    h->computed = true;
    return GENPHI_OK;
}

}  // namespace

extern "C" {

int genphi_carry_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_cases, const int64_t *case_ids,
                        int64_t n_controls, const int64_t *control_ids, int64_t simul_no, uint64_t seed, int32_t panel_cols, int32_t chunk_labels,
                        int32_t max_count, genphi_carry **out)
{
    if (out) *out = nullptr;
    if (int rc = check_create_args("genphi_carry_create", n_ind, ind, father, mother, n_cases, case_ids, n_controls, control_ids, out, INT32_MAX)) return rc;
    if (n_cases == 0) return genphi_set_error(GENPHI_ERR_ARG, "gen.simuCarriers: no cases");
    if (n_cases + n_controls >= INT32_MAX) return genphi_set_error(GENPHI_ERR_ARG, "genphi_carry_create: more than 2^31 - 2 cases and controls");
    if (simul_no < 1 || simul_no > GENPHI_SIMU_MAX_SIMULATIONS)
        return genphi_set_error(GENPHI_ERR_ARG, "gen.simuCarriers: simulNo = " + std::to_string(simul_no) + " is outside 1 .. 2^24");
    if (panel_cols < 0) return genphi_set_error(GENPHI_ERR_ARG, "genphi_carry_create: panel_cols is 0 (the default rule) or positive");
    if (chunk_labels < 0) return genphi_set_error(GENPHI_ERR_ARG, "genphi_carry_create: chunk_labels is 0 (the default rule) or positive");
    if (max_count < 0) return genphi_set_error(GENPHI_ERR_ARG, "genphi_carry_create: max_count is 0 (every count has its column) or positive");
    return create_entry(out, "gen.simuCarriers", [&](genphi_carry *h) {
        h->S = simul_no;
        h->seed = seed;
        h->panel_arg = panel_cols;
        std::vector<int64_t> listed(case_ids, case_ids + n_cases);
        listed.insert(listed.end(), control_ids, control_ids + n_controls);
        std::string err;
        if (const int rc = genphi::plan_ident(h->plan, n_ind, ind, father, mother, static_cast<int64_t>(listed.size()), listed.data(), err))
            return genphi_set_error(rc, err);
        int64_t both_id = 0;
        if (genphi::carry_lists(h->lists, h->plan, n_cases, both_id))
            return genphi_set_error(GENPHI_ERR_ARG, "gen.simuCarriers: " + std::to_string(both_id) + " is listed as a case and as a control");
        h->W = genphi::carry_columns(h->lists.n_cases, max_count);
        const std::string limit = genphi::carry_limits(h->lists.n_cases, h->plan.n_labels, h->W);
        if (!limit.empty()) return genphi_set_error(GENPHI_ERR_ARG, "gen.simuCarriers: " + limit);
        h->chunks = genphi::carry_chunks(h->plan.n_labels, chunk_labels);
        h->panels.set(simul_no, genphi::drop_panel_pairs(simul_no, panel_cols));                // (compute may narrow the default to what fits)
        return GENPHI_OK;
    });
}

int genphi_carry_levels(const genphi_carry *h, int64_t *n_live, int32_t *levels, int64_t *rows_per_level)
{
    return drop_levels(h, "genphi_carry_levels", n_live, levels, rows_per_level);
}

int genphi_carry_alleles(const genphi_carry *h, int64_t *n_labels, int32_t *planes, int64_t *ids, int32_t *sides)
{
    return label_alleles(h, "genphi_carry_alleles", n_labels, planes, ids, sides);
}

int genphi_carry_compute(genphi_carry *h, int32_t device) { return compute_entry(h, device, "genphi_carry_compute", "gen.simuCarriers", compute_impl); }

int genphi_carry_carriers_to_host(genphi_carry *h, int32_t *out)
{
    return result_to_host(h, out, &genphi_carry::d_carriers, "genphi_carry_carriers_to_host", "gen.simuCarriers");
}

int genphi_carry_homozygotes_to_host(genphi_carry *h, int32_t *out)
{
    return result_to_host(h, out, &genphi_carry::d_homozygotes, "genphi_carry_homozygotes_to_host", "gen.simuCarriers");
}

int genphi_carry_excluded_to_host(genphi_carry *h, int32_t *out)
{
    return result_to_host(h, out, &genphi_carry::d_excluded, "genphi_carry_excluded_to_host", "gen.simuCarriers");
}

int genphi_carry_stats(const genphi_carry *h, double *sweep_ms, double *count_ms, double *algorithmic_bytes, double *count_bytes, int32_t *levels,
                       int32_t *panel_cols, int64_t *panels, int32_t *planes, int32_t *chunk_labels, int64_t *chunks, int32_t *lds_bytes, int32_t *columns,
                       int32_t *n_cases, int32_t *n_controls)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_carry_stats: NULL handle");
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
    put(columns, h->W);
    put(n_cases, h->lists.n_cases);
    put(n_controls, h->lists.n_controls);
    return GENPHI_OK;
}

void genphi_carry_destroy(genphi_carry *h) { destroy_entry(h); }

}  // extern "C"
