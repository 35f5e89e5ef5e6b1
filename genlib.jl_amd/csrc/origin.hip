// origin.hip -- gen.simuOrigins: which founder alleles the kinship within and between groups of probands, and their inbreeding, descend
// from, by gene dropping (include/genphi.h, genphi_origin_*).  The label sweep is the shared one (label_sweep.h: the base of the
// handle, the init kernel and the step kernel, on ident's columns: row r, pair j, side s, plane b at ((r * Pn + j) * 2 + s) * B + b,
// 16-byte elements); the plan is ident.h's on the list as given.  Only the reduction is new, and it is the hot path.  It never looks at a
// pair of probands: with k_a gene copies of one label in group a and k_b in group b, the two groups share k_a k_b matching copy pairs.
//   count   one launch per panel after the last level, grid (words of the panel, label chunks), 1,024 threads.  A workgroup owns the
//           64 simulations of one word and the labels [l0, l0 + LC) of one chunk (origin.h: origin_chunks).  It holds 64 tables in
//           LDS, one per simulation, of LC x G counter dwords, (label t, group a) at t G + a: c1 in bits 0-15, c2 in bits 16-30.  Lane s
//           of every wave is simulation s: the lanes of a wave never meet in one dword, only waves do, and those are resolved by 32-bit
//           LDS atomics.  The tables lie stride = (LC G) | 1 dwords apart: for one dword the 64 lanes fall on 64 different banks.
//           1. zero the tables.
//           2. count: wave v takes the individuals i = v, v + 16, .. of the row list (origin.h: the distinct grouped probands, sorted
//              by group), read in place (there is no gather).  The decode is carry.hip's: lane b < B loads its word's half of plane b
//              of side 0 and lane 32 + b that of side 1, one 8-byte load per lane and individual; the two labels of lane s are bit s
//              of the 2 B words, which reach every lane as wave-uniform values (readlane).  Four individuals are loaded before the first
//              is decoded.  A column < S adds into the dwords of its labels that lie in the chunk, at the individual's group: 1 at a
//              and 1 at b, or 0x10001 at a when a = b; then it also adds 1 at autozygous_pro[i, a], when that table is kept.  At most
//              32,767 probands in a group: no field carries into the next.
//           3. reduce, after a barrier, the chunk's labels dealt to the waves: lane s reads the G dwords of its own table.  A label on
//              which no lane has a count (one ballot) is skipped: per simulation at most 2 n of the labels are counted at all.  Else
//              the groups with a count on any lane are found (a ballot per group), and for each of them, and each pair of them, the
//              lane forms k_a = c1 + c2, c2, m_aa = (k_a^2 - c1 - 3 c2) / 2 and m_ab = k_a k_b in 64 bits, the wave sums each over its
//              lanes (a column >= S holds 0), and lane 0 adds the non-zero sums into the Int64 tables.
// Nothing couples neighbouring labels: no halo.  Everything is integer; the only atomics on global memory are integer adds: the same
// bytes on every run, with any panel and chunk.
#include <hip/hip_runtime.h>

#include "origin.h"
#include "label_sweep.h"

namespace {

constexpr int ORIGIN_WAVES = genphi::ORIGIN_THREADS / 64;
constexpr int ORIGIN_UNROLL = 4;             // individuals a wave has in flight

// The sum of v over the 64 lanes, in every lane.
__device__ __forceinline__ u64 wave_sum(u64 v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ void add64(long long *cell, u64 v) { atomicAdd(reinterpret_cast<unsigned long long *>(cell), static_cast<unsigned long long>(v)); }

// Block (blockIdx.x, blockIdx.y): word blockIdx.x of the panel (pair blockIdx.x >> 1, its x or y half) and chunk chunk0 + blockIdx.y.
// lists: the rows, the groups and the positions of the n_ind individuals of the row list, n_ind entries each.
__global__ void __launch_bounds__(genphi::ORIGIN_THREADS)
origin_count_kernel(const ulonglong2 *__restrict__ rows, const int *__restrict__ lists, int n_ind, long long n_labels, int Pn, int B, long long first_pair,
                    long long S, long long chunk0, int LC, int G, int stride, long long *__restrict__ copies, long long *__restrict__ autozygous,
                    long long *__restrict__ matches, int *__restrict__ by_pro)
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

    for (int i = threadIdx.x; i < 64 * stride; i += genphi::ORIGIN_THREADS) tables[i] = 0u;
    __syncthreads();

    // ---- count ----
    const int *ind_row = lists, *ind_group = lists + n_ind, *ind_index = lists + 2 * n_ind;
    const u64 *halves = reinterpret_cast<const u64 *>(rows) + (word & 1);
    const long long pair = word >> 1;
    const int side = lane >> 5, plane = lane & 31;
    unsigned *mine = tables + lane * stride;
    for (int i0 = wave; i0 < n_ind; i0 += ORIGIN_WAVES * ORIGIN_UNROLL) {
        unsigned lo[ORIGIN_UNROLL], hi[ORIGIN_UNROLL];
#pragma unroll
        for (int q = 0; q < ORIGIN_UNROLL; ++q) {
            const int i = i0 + q * ORIGIN_WAVES;
            u64 w = 0;
            if (i < n_ind && plane < B) {
                const long long e = ((static_cast<long long>(ind_row[i]) * Pn + pair) * 2 + side) * B + plane;
                w = halves[2 * e];
            }
            lo[q] = static_cast<unsigned>(w);
            hi[q] = static_cast<unsigned>(w >> 32);
        }
#pragma unroll
        for (int q = 0; q < ORIGIN_UNROLL; ++q) {
            const int i = i0 + q * ORIGIN_WAVES;
            if (i >= n_ind) break;                                       // (uniform)
            unsigned a = 0, b = 0;
            for (int p = 0; p < B; ++p) {
                const unsigned al = __builtin_amdgcn_readlane(lo[q], p), ah = __builtin_amdgcn_readlane(hi[q], p);
                const unsigned bl = __builtin_amdgcn_readlane(lo[q], 32 + p), bh = __builtin_amdgcn_readlane(hi[q], 32 + p);
                a |= (((lane < 32 ? al : ah) >> (lane & 31)) & 1u) << p;
                b |= (((lane < 32 ? bl : bh) >> (lane & 31)) & 1u) << p;
            }
            const int g = ind_group[i];                                  // (uniform)
            const long long ra = static_cast<long long>(a) - l0, rb = static_cast<long long>(b) - l0;
            const bool in_a = live_col && ra >= 0 && ra < own, in_b = live_col && b != a && rb >= 0 && rb < own;
            if (in_a) atomicAdd(mine + ra * G + g, a == b ? 0x10001u : 1u);
            if (in_b) atomicAdd(mine + rb * G + g, 1u);
            if (by_pro && in_a && a == b) atomicAdd(by_pro + (static_cast<long long>(ind_index[i]) * n_labels + a), 1);
        }
    }
    __syncthreads();

    // ---- reduce ----
    for (int t = wave; t < own; t += ORIGIN_WAVES) {
        const unsigned *cell = mine + t * G;
        unsigned any = 0;
        if (live_col)
            for (int a = 0; a < G; ++a) any |= cell[a];
        if (__ballot(any != 0) == 0) continue;                           // (uniform) nobody carries this label in these simulations
        unsigned groups = 0;                                             // (uniform) the groups with a count on some lane
        for (int a = 0; a < G; ++a)
            if (__ballot(live_col && cell[a] != 0) != 0) groups |= 1u << a;
        const long long l = l0 + t;
        for (unsigned ma = groups; ma; ma &= ma - 1) {
            const int a = __ffs(ma) - 1;
            const unsigned v = live_col ? cell[a] : 0u;
            const u64 c1 = v & 0xFFFFu, c2 = (v >> 16) & 0x7FFFu, k = c1 + c2;
            const u64 sum_k = wave_sum(k), sum_2 = wave_sum(c2), sum_m = wave_sum((k * k - c1 - 3 * c2) >> 1);
            const long long p_aa = static_cast<long long>(a) * G - static_cast<long long>(a) * (a - 1) / 2;
            if (lane == 0) {
                add64(copies + (a * n_labels + l), sum_k);
                if (sum_2) add64(autozygous + (a * n_labels + l), sum_2);
                if (sum_m) add64(matches + (p_aa * n_labels + l), sum_m);
            }
            for (unsigned mb = ma & (ma - 1); mb; mb &= mb - 1) {
                const int b = __ffs(mb) - 1;
                const unsigned vb = live_col ? cell[b] : 0u;
                const u64 kb = (vb & 0xFFFFu) + ((vb >> 16) & 0x7FFFu);
                const u64 sum_ab = wave_sum(k * kb);
                if (sum_ab && lane == 0) add64(matches + ((p_aa + (b - a)) * n_labels + l), sum_ab);
            }
        }
    }
}

}  // namespace

struct genphi_origin : LabelSweep {          // d_slots: the rows of one panel (n_live x pairs x 2 sides x B planes x 16 bytes)
    genphi::OriginLists lists;               // the row list (origin.h)
    genphi::OriginChunks chunks;             // the chunk rule (origin.h)
    int32_t G = 1;
    bool by_proband = false;
    DevBuf<int> d_lists, d_by_pro;           // d_lists: the rows, the groups and the positions of the row list, n entries each
    DevBuf<long long> d_copies, d_autozygous, d_matches;
    DropPanels panels;
    double count_ms = 0.0, count_bytes = 0.0;
    genphi_origin() { own(d_lists, d_by_pro, d_copies, d_autozygous, d_matches); }
};

namespace {

// The panel width, the rows, the results and the lists on the device; GENPHI_ERR_ALLOC before any launch.
int prepare(genphi_origin *h)
{
    const genphi::IdentPlan &pl = h->plan;
    const genphi::OriginSizes z = genphi::origin_sizes(pl, h->lists, h->G, h->by_proband);
    double usable = 0.0;
    if (int rc = h->usable_bytes(usable, h->held_bytes())) return rc;
    const double room = usable - static_cast<double>(z.fixed()) - (64 << 20);
    const double pair_bytes = static_cast<double>(z.panel(1));
    int64_t Pn;
    if (!genphi::drop_panel_fits(Pn, h->S, h->panel_arg, room, pair_bytes))
        return genphi_set_error(GENPHI_ERR_ALLOC, "gen.simuOrigins: the tables of " + std::to_string(pl.n_labels) + " founder alleles and " + std::to_string(h->G) +
                                                      " groups, the lists and " + std::to_string(pl.n_live) + " live rows of " + std::to_string(pl.planes) +
                                                      " planes and " + std::to_string(128 * std::max<int64_t>(Pn, 1)) + " simulations do not fit on device " +
                                                      std::to_string(h->device));
    GENPHI_HIP_TRY(h->d_slots.reserve(z.pair_rows * static_cast<size_t>(Pn)));
    GENPHI_HIP_TRY(h->d_copies.reserve(z.copies / 8));
    GENPHI_HIP_TRY(h->d_autozygous.reserve(z.autozygous / 8));
    GENPHI_HIP_TRY(h->d_matches.reserve(z.matches / 8));
    if (h->by_proband) GENPHI_HIP_TRY(h->d_by_pro.reserve(z.by_proband / 4));
    if (int rc = h->upload_lists()) return rc;
    std::vector<int32_t> packed(h->lists.rows);
    packed.insert(packed.end(), h->lists.group.begin(), h->lists.group.end());
    packed.insert(packed.end(), h->lists.index.begin(), h->lists.index.end());
    if (int rc = h->upload(h->d_lists, packed)) return rc;
    GENPHI_HIP_TRY(hipStreamSynchronize(h->stream));                     // (packed is a local)
    h->panels.set(h->S, Pn);
    return GENPHI_OK;
}

int compute_impl(genphi_origin *h, int32_t device)
{
    if (int rc = h->select(device)) return rc;
    if (int rc = prepare(h)) return rc;
    const genphi::IdentPlan &pl = h->plan;
    const genphi::OriginChunks &ch = h->chunks;
    const int Pn = h->panels.pairs, B = pl.planes, n_ind = static_cast<int>(h->lists.n);
    const int64_t total = h->panels.total;
    ulonglong2 *rows = h->slots<ulonglong2>();
    if (ch.lds_bytes > 32768)
        GENPHI_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(origin_count_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           static_cast<int>(ch.lds_bytes)));
    PhaseTimer timer;
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_copies.get(), 0, h->d_copies.bytes(), h->stream));
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_autozygous.get(), 0, h->d_autozygous.bytes(), h->stream));
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_matches.get(), 0, h->d_matches.bytes(), h->stream));
    if (h->by_proband) GENPHI_HIP_TRY(hipMemsetAsync(h->d_by_pro.get(), 0, h->d_by_pro.bytes(), h->stream));
    double sweep_ms = 0.0, count_ms = 0.0;
    int64_t launches = 0;
    for (int64_t p0 = 0; p0 < total; p0 += Pn) {
        const int Pc = static_cast<int>(std::min<int64_t>(Pn, total - p0));
        if (int rc = timer.begin(h->stream)) return rc;
        if (int rc = label_sweep_panel(h, Pc, static_cast<unsigned>(p0))) return rc;
        if (int rc = timer.middle(h->stream)) return rc;
        for (int64_t c0 = 0; c0 < ch.chunks; c0 += 65535) {          // (a grid's y extent)
            const dim3 grid(static_cast<unsigned>(2 * Pc), static_cast<unsigned>(std::min<int64_t>(65535, ch.chunks - c0)));
            origin_count_kernel<<<grid, genphi::ORIGIN_THREADS, ch.lds_bytes, h->stream>>>(rows, h->d_lists.get(), n_ind, pl.n_labels, Pn, B, p0, h->S, c0,
                                                                                           static_cast<int>(ch.chunk_labels), h->G, ch.stride, h->d_copies.get(),
                                                                                           h->d_autozygous.get(), h->d_matches.get(),
                                                                                           h->by_proband ? h->d_by_pro.get() : nullptr);
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

int genphi_origin_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro, const int64_t *pro_ids,
                         const int32_t *group, int32_t n_groups, int64_t simul_no, uint64_t seed, int32_t panel_cols, int32_t chunk_labels, int32_t by_proband,
                         genphi_origin **out)
{
    if (out) *out = nullptr;
    if (int rc = check_create_args("genphi_origin_create", n_ind, ind, father, mother, n_pro, pro_ids, 0, nullptr, out, 0)) return rc;
    if (n_pro == 0) return genphi_set_error(GENPHI_ERR_ARG, "gen.simuOrigins: no probands");
    if (n_groups < 1 || n_groups > genphi::ORIGIN_MAX_GROUPS)
        return genphi_set_error(GENPHI_ERR_ARG, "gen.simuOrigins: " + std::to_string(n_groups) + " groups; 1 .. 32 are taken");
    if (!group && n_groups != 1) return genphi_set_error(GENPHI_ERR_ARG, "genphi_origin_create: group is NULL (everyone in group 0) but n_groups is not 1");
    if (simul_no < 1 || simul_no > GENPHI_SIMU_MAX_SIMULATIONS)
        return genphi_set_error(GENPHI_ERR_ARG, "gen.simuOrigins: simulNo = " + std::to_string(simul_no) + " is outside 1 .. 2^24");
    if (panel_cols < 0) return genphi_set_error(GENPHI_ERR_ARG, "genphi_origin_create: panel_cols is 0 (the default rule) or positive");
    if (chunk_labels < 0) return genphi_set_error(GENPHI_ERR_ARG, "genphi_origin_create: chunk_labels is 0 (the default rule) or positive");
    if (by_proband != 0 && by_proband != 1) return genphi_set_error(GENPHI_ERR_ARG, "genphi_origin_create: by_proband is 0 or 1");
    return create_entry(out, "gen.simuOrigins", [&](genphi_origin *h) {
        h->S = simul_no;
        h->seed = seed;
        h->panel_arg = panel_cols;
        h->G = n_groups;
        h->by_proband = by_proband != 0;
        std::string err;
        if (const int rc = genphi::plan_ident(h->plan, n_ind, ind, father, mother, n_pro, pro_ids, err)) return genphi_set_error(rc, err);
        int64_t bad = 0;
        switch (genphi::origin_lists(h->lists, h->plan, group, n_groups, bad)) {
        case genphi::ORIGIN_LIST_RANGE:
            return genphi_set_error(GENPHI_ERR_ARG, "gen.simuOrigins: the group of list entry " + std::to_string(bad) + " is outside -1 .. " + std::to_string(n_groups - 1));
        case genphi::ORIGIN_LIST_CONFLICT:
            return genphi_set_error(GENPHI_ERR_ARG, "gen.simuOrigins: " + std::to_string(bad) + " is listed with two different groups");
        default:
            break;
        }
        const std::string limit = genphi::origin_limits(h->lists, h->plan.n_labels, h->by_proband);
        if (!limit.empty()) return genphi_set_error(GENPHI_ERR_ARG, "gen.simuOrigins: " + limit);
        h->chunks = genphi::origin_chunks(h->plan.n_labels, n_groups, chunk_labels);
        h->panels.set(simul_no, genphi::drop_panel_pairs(simul_no, panel_cols));                // (compute may narrow the default to what fits)
        return GENPHI_OK;
    });
}

int genphi_origin_levels(const genphi_origin *h, int64_t *n_live, int32_t *levels, int64_t *rows_per_level)
{
    return drop_levels(h, "genphi_origin_levels", n_live, levels, rows_per_level);
}

int genphi_origin_alleles(const genphi_origin *h, int64_t *n_labels, int32_t *planes, int64_t *ids, int32_t *sides)
{
    return label_alleles(h, "genphi_origin_alleles", n_labels, planes, ids, sides);
}

int genphi_origin_compute(genphi_origin *h, int32_t device) { return compute_entry(h, device, "genphi_origin_compute", "gen.simuOrigins", compute_impl); }

int genphi_origin_copies_to_host(genphi_origin *h, int64_t *out)
{
    return result_to_host(h, out, &genphi_origin::d_copies, "genphi_origin_copies_to_host", "gen.simuOrigins");
}

int genphi_origin_autozygous_to_host(genphi_origin *h, int64_t *out)
{
    return result_to_host(h, out, &genphi_origin::d_autozygous, "genphi_origin_autozygous_to_host", "gen.simuOrigins");
}

int genphi_origin_matches_to_host(genphi_origin *h, int64_t *out)
{
    return result_to_host(h, out, &genphi_origin::d_matches, "genphi_origin_matches_to_host", "gen.simuOrigins");
}

int genphi_origin_by_proband_to_host(genphi_origin *h, int32_t *out)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_origin_by_proband_to_host: NULL handle");
    if (!h->by_proband) return genphi_set_error(GENPHI_ERR_ARG, "genphi_origin_by_proband_to_host: the handle was created without by_proband");
    return result_to_host(h, out, &genphi_origin::d_by_pro, "genphi_origin_by_proband_to_host", "gen.simuOrigins");
}

int genphi_origin_stats(const genphi_origin *h, double *sweep_ms, double *count_ms, double *algorithmic_bytes, double *count_bytes, int32_t *levels,
                        int32_t *panel_cols, int64_t *panels, int32_t *planes, int32_t *chunk_labels, int64_t *chunks, int32_t *lds_bytes, int32_t *n_groups,
                        int32_t *n_grouped)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_origin_stats: NULL handle");
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
    put(n_groups, h->G);
    put(n_grouped, h->lists.n);
    return GENPHI_OK;
}

void genphi_origin_destroy(genphi_origin *h) { destroy_entry(h); }

}  // extern "C"
