// ident.hip -- gen.simuIdentity: Jacquard's nine condensed identity states by gene dropping (include/genphi.h, genphi_ident_*).
//
// Every founder allele is dropped under its own label.  A label has B bits, so a side of an individual is B bit rows over the
// simulations (plane b holds bit b of the label in every simulation), 64 simulations per word, and a meiosis is
// (T & P_parent[b]) | (~T & M_parent[b]) for all B planes with ONE random word T: the word of gen.simuSample (simu.hip), keyed
// on (seed, ID, side, absolute pair index).  The host plan (ident.h, no GPU) lists the live set by level and the allele table.
//   layout  a panel row holds Pn pairs of words; the B planes of one (row, pair, side) are contiguous 16-byte elements and the
//           two sides of a pair are neighbours: row r, pair j, side s, plane b at ((r * Pn + j) * 2 + s) * B + b (ulonglong2)
//   (init, step and gather live in label_sweep.h with the base of the handle: retain.hip and link.hip sweep with them too)
//   init    the sides with an unknown parent, at any level: plane b of label k is all ones or all zeros.  Only these are ever
//           initialised: every other side is written whole by the step of its row's level before anything reads it
//   step    one launch per level >= 1: LPR lanes per row, a lane owns a pair of words: per known side one Philox block and the
//           two contiguous runs of B planes of that parent; 16-byte loads and stores
//   gather  the listed probands' rows in list order, transposed: pair j, side s, plane b, proband i at ((j * 2 + s) * B + b) *
//           n_pro + i, so a tile of the pair kernel is B * 2 contiguous runs of 32 elements for its rows and for its columns
//   pair    the hot path.  A workgroup of 256 threads owns a tile of 32 x 32 ordered pairs (i, j) and walks the pairs of words
//           of the panel: it stages the planes of its 32 rows and 32 columns in LDS (2048 * B bytes), a thread owns 2 x 2 pairs
//           and keeps 8 counters per pair in registers (the ninth state is the panel's columns minus the rest).  Per word it
//           ORs x_b ^ y_b over the planes into six inequality words per pair (ab, cd, ac, ad, bc, bd; ab and cd once per row
//           and column of its 2 x 2), masks the equality words to the columns < S, forms the state words and adds popcounts.
//           Shipped form: the tiles with tile row <= tile column; an off-diagonal tile also adds its counts to the mirrored
//           pairs with the states 3 <-> 5 and 4 <-> 6 exchanged.  GENPHI_IDENT_FLAG_ALL_PAIRS computes every tile instead
//           (the A/B of profiles/ident_bench.py).  A pair has one owner per panel and panels run one after the other on one
//           stream: plain Int32 adds, no atomics
//   labels  under GENPHI_IDENT_FLAG_LABELS: a lane per column expands the planes of the listed probands into Int32
// Everything is integer and keyed on IDs and absolute word indices: the same bytes on every run, with any panel width.
#include <hip/hip_runtime.h>

#include "label_sweep.h"

namespace {

constexpr int IDENT_TILE = 32;               // the pair kernel's tile: 32 rows x 32 columns, 2 x 2 pairs per thread

// The 32 x 32 tile (blockIdx.y, blockIdx.x) of ordered pairs over the Pc pairs of words of a panel (see the head of the file).
// tile[]: word w of the pair, side s, plane b, then 64 entries: the tile's 32 rows and its 32 columns.  Thread (ty, tx) owns the
// rows ty, ty + 16 and the columns tx, tx + 16: a wave reads 4 row addresses (broadcast) and 16 consecutive column entries.
__global__ void __launch_bounds__(256)
ident_pair_kernel(const ulonglong2 *__restrict__ gathered, int n_pro, int B, int Pc, long long first_pair, long long S, int mirror,
                  int *__restrict__ counts)
{
    extern __shared__ u64 tile[];
    const int tr = blockIdx.y, tc = blockIdx.x;
    if (mirror && tr > tc) return;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int B2 = 2 * B;
    int cnt[2][2][8];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int k = 0; k < 8; ++k) cnt[r][c][k] = 0;
    for (int p = 0; p < Pc; ++p) {
        __syncthreads();                                 // the previous pair of words has been read
        for (int e = t; e < B2 * 64; e += 256) {
            const int idx = e & 63, q = e >> 6;
            const int g = idx < IDENT_TILE ? tr * IDENT_TILE + idx : tc * IDENT_TILE + idx - IDENT_TILE;
            ulonglong2 v = make_ulonglong2(0, 0);
            if (g < n_pro) v = gathered[(static_cast<long long>(p) * B2 + q) * n_pro + g];
            tile[q * 64 + idx] = v.x;
            tile[(B2 + q) * 64 + idx] = v.y;
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const u64 mask = column_mask(S, 2 * (first_pair + p) + w);
            if (mask == 0) continue;                     // (uniform) the last pair's second word holds no column < S
            const u64 *P = tile + w * B2 * 64, *M = P + B * 64;
            u64 nab[2] = {0, 0}, ncd[2] = {0, 0}, nac[2][2] = {{0, 0}, {0, 0}}, nad[2][2] = {{0, 0}, {0, 0}}, nbc[2][2] = {{0, 0}, {0, 0}},
                nbd[2][2] = {{0, 0}, {0, 0}};
            for (int b = 0; b < B; ++b) {
                u64 a[2], bb[2], c[2], d[2];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    a[r] = P[b * 64 + ty + 16 * r];
                    bb[r] = M[b * 64 + ty + 16 * r];
                    c[r] = P[b * 64 + IDENT_TILE + tx + 16 * r];
                    d[r] = M[b * 64 + IDENT_TILE + tx + 16 * r];
                    nab[r] |= a[r] ^ bb[r];
                    ncd[r] |= c[r] ^ d[r];
                }
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        nac[r][k] |= a[r] ^ c[k];
                        nad[r][k] |= a[r] ^ d[k];
                        nbc[r][k] |= bb[r] ^ c[k];
                        nbd[r][k] |= bb[r] ^ d[k];
                    }
            }
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    // every counted state has an unnegated equality word as a factor: masking those masks the states
                    const u64 ab = ~nab[r] & mask, cd = ~ncd[k] & mask, ac = ~nac[r][k] & mask, ad = ~nad[r][k] & mask,
                              bc = ~nbc[r][k] & mask, bd = ~nbd[r][k] & mask;
                    const u64 both = ab & cd, i_only = ab & ~cd, j_only = cd & ~ab;
                    const u64 i_in_j = ac | ad, j_in_i = ac | bc;
                    const u64 two = (ac & bd) | (ad & bc), any = ac | ad | bc | bd;
                    const u64 s8 = any & ~two & ~ab & ~cd, s7 = two & ~ab & ~cd;
                    int *n = cnt[r][k];
                    n[0] += __popcll(both & ac);
                    n[1] += __popcll(both & ~ac);
                    n[2] += __popcll(i_only & i_in_j);
                    n[3] += __popcll(i_only & ~i_in_j);
                    n[4] += __popcll(j_only & j_in_i);
                    n[5] += __popcll(j_only & ~j_in_i);
                    n[6] += __popcll(s7);
                    n[7] += __popcll(s8);
                }
        }
    }
    const long long col0 = 128 * first_pair;
    const int valid = static_cast<int>(min(S, col0 + 128ll * Pc) - col0);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = tr * IDENT_TILE + ty + 16 * r, j = tc * IDENT_TILE + tx + 16 * k;
            if (i >= n_pro || j >= n_pro) continue;
            const int *n = cnt[r][k];
            const int ninth = valid - (n[0] + n[1] + n[2] + n[3] + n[4] + n[5] + n[6] + n[7]);
            int *o = counts + (static_cast<long long>(i) * n_pro + j) * 9;
#pragma unroll
            for (int s = 0; s < 8; ++s) o[s] += n[s];
            o[8] += ninth;
            if (mirror && tr != tc) {                    // (j, i): the roles of the two individuals exchanged
                int *q = counts + (static_cast<long long>(j) * n_pro + i) * 9;
                q[0] += n[0]; q[1] += n[1]; q[2] += n[4]; q[3] += n[5]; q[4] += n[2]; q[5] += n[3]; q[6] += n[6]; q[7] += n[7];
                q[8] += ninth;
            }
        }
}

// labels[i][side][column]: a lane per column of a word, a wave per (proband, side, word); columns >= S are dropped at the store.
__global__ void __launch_bounds__(256)
ident_label_kernel(const ulonglong2 *__restrict__ gathered, int n_pro, int B, int Wc, long long first_word, long long S, int *__restrict__ labels)
{
    const long long t = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const int bit = static_cast<int>(t & 63);
    const long long u = t >> 6;                          // (proband * 2 + side) * Wc + word
    if (u >= 2ll * n_pro * Wc) return;
    const int w = static_cast<int>(u % Wc);
    const long long is = u / Wc;
    const long long col = 64 * (first_word + w) + bit;
    if (col >= S) return;
    const ulonglong2 *src = gathered + ((static_cast<long long>(w >> 1) * 2 + (is & 1)) * B) * n_pro + (is >> 1);
    int label = 0;
    for (int b = 0; b < B; ++b) {
        const ulonglong2 v = src[static_cast<long long>(b) * n_pro];
        label |= static_cast<int>(((w & 1 ? v.y : v.x) >> bit) & 1) << b;
    }
    labels[is * S + col] = label;
}

}  // namespace

struct genphi_ident : LabelSweep {           // d_slots: the rows of one panel (n_live x pairs x 2 sides x B planes x 16 bytes)
    bool want_labels = false, all_pairs = false;
    DevBuf<int> d_counts, d_labels;
    DevBuf<ulonglong2> d_gathered;           // the listed probands' rows of one panel, transposed (label_gather_kernel)
    DropPanels panels;
    double pair_ms = 0.0, word_ops = 0.0;
    genphi_ident() { own(d_counts, d_labels, d_gathered); }
};

namespace {

// The panel width, the rows, the results and the lists on the device; GENPHI_ERR_ALLOC before any launch.
int prepare(genphi_ident *h)
{
    const genphi::IdentPlan &pl = h->plan;
    const genphi::IdentSizes z = genphi::ident_sizes(pl, h->S, h->want_labels);
    double usable = 0.0;
    if (int rc = h->usable_bytes(usable, h->held_bytes())) return rc;
    const double room = usable - static_cast<double>(z.fixed()) - (64 << 20);
    const double pair_bytes = static_cast<double>(z.panel(1));
    int64_t Pn;
    if (!genphi::drop_panel_fits(Pn, h->S, h->panel_arg, room, pair_bytes))
        return genphi_set_error(GENPHI_ERR_ALLOC, "gen.simuIdentity: the counts of " + std::to_string(pl.n_pro) + " probands" +
                                                      (h->want_labels ? ", the labels" : "") + " and " + std::to_string(pl.n_live) + " live rows of " +
                                                      std::to_string(pl.planes) + " planes and " + std::to_string(128 * std::max<int64_t>(Pn, 1)) +
                                                      " simulations do not fit on device " + std::to_string(h->device));
    GENPHI_HIP_TRY(h->d_slots.reserve(z.pair_rows * static_cast<size_t>(Pn)));
    GENPHI_HIP_TRY(h->d_gathered.reserve(z.pair_gather * static_cast<size_t>(Pn) / sizeof(ulonglong2)));
    GENPHI_HIP_TRY(h->d_counts.reserve(z.counts / 4));
    if (h->want_labels) GENPHI_HIP_TRY(h->d_labels.reserve(z.labels / 4));
    if (int rc = h->upload_lists()) return rc;
    h->panels.set(h->S, Pn);
    return GENPHI_OK;
}

int compute_impl(genphi_ident *h, int32_t device)
{
    if (int rc = h->select(device)) return rc;
    if (int rc = prepare(h)) return rc;
    const genphi::IdentPlan &pl = h->plan;
    const int Pn = h->panels.pairs, B = pl.planes, n_pro = static_cast<int>(pl.n_pro);
    const int64_t total = h->panels.total;
    const unsigned tiles = static_cast<unsigned>((n_pro + IDENT_TILE - 1) / IDENT_TILE);
    const size_t lds = static_cast<size_t>(2 * 2 * 64 * 8) * static_cast<size_t>(B);
    PhaseTimer timer;
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_counts.get(), 0, h->d_counts.bytes(), h->stream));
    double sweep_ms = 0.0, pair_ms = 0.0;
    int64_t launches = 0;
    for (int64_t p0 = 0; p0 < total; p0 += Pn) {
        const int Pc = static_cast<int>(std::min<int64_t>(Pn, total - p0));
        if (int rc = timer.begin(h->stream)) return rc;
        if (int rc = label_sweep_panel(h, Pc, static_cast<unsigned>(p0))) return rc;
        if (int rc = timer.middle(h->stream)) return rc;
        if (int rc = h->gather_panel(Pn, Pc, h->d_gathered.get())) return rc;
        ident_pair_kernel<<<dim3(tiles, tiles), 256, lds, h->stream>>>(h->d_gathered.get(), n_pro, B, Pc, p0, h->S, h->all_pairs ? 0 : 1, h->d_counts.get());
        GENPHI_HIP_TRY(hipGetLastError());
        if (int rc = timer.end(h->stream)) return rc;
        if (h->want_labels) {
            const long long threads = 2ll * n_pro * (2 * Pc) * 64;
            ident_label_kernel<<<static_cast<unsigned>((threads + 255) / 256), 256, 0, h->stream>>>(h->d_gathered.get(), n_pro, B, 2 * Pc, 2 * p0, h->S,
                                                                                                   h->d_labels.get());
            GENPHI_HIP_TRY(hipGetLastError());
        }
        if (int rc = timer.add(sweep_ms, pair_ms)) return rc;
        launches += pl.n_levels + 2 + (h->want_labels ? 1 : 0);
    }
    GENPHI_HIP_TRY(hipStreamSynchronize(h->stream));
    // per side with a known parent: two runs of B planes read and one written, 16 bytes per plane and pair of words, over the panels
    const double known_sides = 2.0 * static_cast<double>(pl.n_live) - static_cast<double>(pl.n_labels);
    const double n = static_cast<double>(n_pro);
    h->sweep_ms = sweep_ms;
    h->pair_ms = pair_ms;
    h->alg_bytes = 3.0 * 16.0 * B * known_sides * static_cast<double>(total);
    h->word_ops = (h->all_pairs ? n * n : n * (n + 1.0) / 2.0) * static_cast<double>((h->S + 63) / 64) * (12.0 * B + 40.0);
    h->n_launches = launches;
    h->computed = true;
    return GENPHI_OK;
}

}  // namespace

extern "C" {

int genphi_ident_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro, const int64_t *pro_ids,
                        int64_t simul_no, uint64_t seed, int32_t panel_cols, int32_t flags, genphi_ident **out)
{
    if (out) *out = nullptr;
    if (out && (flags & ~(GENPHI_IDENT_FLAG_LABELS | GENPHI_IDENT_FLAG_ALL_PAIRS))) return genphi_set_error(GENPHI_ERR_ARG, "genphi_ident_create: unknown flag");
    if (int rc = check_create_args("genphi_ident_create", n_ind, ind, father, mother, n_pro, pro_ids, 0, nullptr, out, 0)) return rc;
    if (n_pro == 0) return genphi_set_error(GENPHI_ERR_ARG, "gen.simuIdentity: no probands");
    if (n_pro * n_pro >= (int64_t(1) << 31))
        return genphi_set_error(GENPHI_ERR_ARG, "gen.simuIdentity: " + std::to_string(n_pro) + " probands: 2^31 or more ordered pairs");
    if (simul_no < 1 || simul_no > GENPHI_SIMU_MAX_SIMULATIONS)
        return genphi_set_error(GENPHI_ERR_ARG, "gen.simuIdentity: simulNo = " + std::to_string(simul_no) + " is outside 1 .. 2^24");
    if (panel_cols < 0) return genphi_set_error(GENPHI_ERR_ARG, "genphi_ident_create: panel_cols is 0 (the default rule) or positive");
    return create_entry(out, "gen.simuIdentity", [&](genphi_ident *h) {
        h->S = simul_no;
        h->seed = seed;
        h->want_labels = (flags & GENPHI_IDENT_FLAG_LABELS) != 0;
        h->all_pairs = (flags & GENPHI_IDENT_FLAG_ALL_PAIRS) != 0;
        h->panel_arg = panel_cols;
        std::string err;
        if (const int rc = genphi::plan_ident(h->plan, n_ind, ind, father, mother, n_pro, pro_ids, err)) return genphi_set_error(rc, err);
        h->panels.set(simul_no, genphi::drop_panel_pairs(simul_no, panel_cols));                // (compute may narrow the default to what fits)
        return GENPHI_OK;
    });
}

int genphi_ident_levels(const genphi_ident *h, int64_t *n_live, int32_t *levels, int64_t *rows_per_level)
{
    return drop_levels(h, "genphi_ident_levels", n_live, levels, rows_per_level);
}

int genphi_ident_alleles(const genphi_ident *h, int64_t *n_labels, int32_t *planes, int64_t *ids, int32_t *sides)
{
    return label_alleles(h, "genphi_ident_alleles", n_labels, planes, ids, sides);
}

int genphi_ident_compute(genphi_ident *h, int32_t device) { return compute_entry(h, device, "genphi_ident_compute", "gen.simuIdentity", compute_impl); }

int genphi_ident_counts_to_host(genphi_ident *h, int32_t *out)
{
    return result_to_host(h, out, &genphi_ident::d_counts, "genphi_ident_counts_to_host", "gen.simuIdentity");
}

int genphi_ident_labels_to_host(genphi_ident *h, int32_t *out)
{
    return labels_to_host(h, out, "genphi_ident_labels_to_host", "GENPHI_IDENT_FLAG_LABELS", "gen.simuIdentity");
}

int genphi_ident_stats(const genphi_ident *h, double *sweep_ms, double *pair_ms, double *algorithmic_bytes, double *word_ops, int32_t *levels,
                       int32_t *panel_cols, int64_t *panels, int32_t *planes, int32_t *tile_rows, int32_t *tile_cols, int32_t *lanes_per_row)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_ident_stats: NULL handle");
    h->stats(sweep_ms, algorithmic_bytes, nullptr);
    put(pair_ms, h->pair_ms);
    put(word_ops, h->word_ops);
    put(levels, h->plan.n_levels);
    put(panel_cols, 128 * h->panels.pairs);
    put(panels, h->panels.n_panels);
    put(planes, h->plan.planes);
    put(tile_rows, IDENT_TILE);
    put(tile_cols, IDENT_TILE);
    put(lanes_per_row, h->panels.lanes_per_row);
    return GENPHI_OK;
}

void genphi_ident_destroy(genphi_ident *h) { destroy_entry(h); }

}  // extern "C"
