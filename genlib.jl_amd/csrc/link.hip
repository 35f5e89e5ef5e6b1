// link.hip -- gen.simuSharing: linked-locus gene dropping and identity by descent along a chromosome (include/genphi.h, genphi_link_*).
//
// gen.simuIdentity (ident.hip) drops every founder allele under its own label at ONE locus: a side is B bit rows over the simulations.
// Here a simulation is a whole chromosome of L loci, W = ceil(L / 64) words: a side is B bit rows over (simulation, locus), and a
// meiosis copies a mosaic of the parent's two chromosomes: (T & P_parent[b]) | (~T & M_parent[b]) with the transmission word T = the
// prefix XOR of the crossover words X along the chromosome (link.h).  The host plan is ident's (ident.h), unchanged.
//   layout  ident's, with the column index of a panel row running over (simulation, pair of words), the pair fastest: row r, column
//           c = s * Wp + p, side, plane b at ((r * Cn + c) * 2 + side) * B + b (ulonglong2: the words 2p and 2p + 1 of the chromosome)
//   (init and gather live in label_sweep.h with the base of the handle; ident.hip and retain.hip use them too)
//   init    the sides with an unknown parent, as in ident: plane b of label k is all ones or all zeros
//   step    one launch per level >= 1 and panel.  LPS = the power of two >= Wp lanes own the pairs of words of one simulation of one
//           row and are neighbours in a wave (Wp <= 32: a simulation never spans waves).  A lane draws and folds its own two X words
//           per known side; the parity of all earlier words of the simulation reaches it by a segmented XOR scan over those lanes
//           (wave shuffles), both sides in one scan; inside a word the prefix is six shift-and-XOR steps.  One T serves all B planes
//           of a side; 16-byte loads and stores
//   gather  the listed probands' rows in list order, transposed as in ident: column c, side, plane b, proband i at ((c * 2 + side) *
//           B + b) * n_pro + i
//   pair    the hot path.  ident's tiling: a workgroup of 256 threads owns 32 x 32 pairs (i, j), a thread 2 x 2 of them; it stages the
//           planes of its 32 rows and 32 columns of one pair of words in LDS (2048 * B bytes).  The walk is simulation-major: per
//           word the four equality words ac, ad, bc, bd from the planes, masked to the loci < L, then any and two; popcounts into the
//           simulation's m, n1, n2 and the runs of `any` as popcount(any & ~(any << 1 | carry)), the carry being bit 63 of the
//           previous word's `any` of the same simulation.  At the end of a simulation m, m * m, n1, n2, g and [n1 > 0] go to the
//           thread's six Int64 accumulators.  Shipped form: the tiles with tile row <= tile column; an off-diagonal tile also adds
//           its sums to the mirrored pairs (all six are symmetric).  GENPHI_LINK_FLAG_ALL_PAIRS computes every tile instead.  A pair
//           has one owner per panel and panels run one after the other on one stream: plain Int64 adds, no atomics
//   labels  under GENPHI_LINK_FLAG_LABELS: a lane per locus of a word expands the planes of the listed probands into Int32
//   segment under a request (genphi_seg_*, gen.simuSegments): after the pair kernel, on its tile and staging, the lengths of the runs of
//           `any`: a state carried from word to word (link_segments.h), a table of 64-bit counters in LDS, Int64 per pair
// Everything is integer and keyed on IDs and absolute simulation and word indices: the same bytes on every run, with any panel width.
#include <hip/hip_runtime.h>

#include <vector>

#include "label_sweep.h"
#include "link.h"
#include "link_segments.h"

namespace {

constexpr int LINK_TILE = 32;                // the pair kernel's tile: 32 rows x 32 columns, 2 x 2 pairs per thread

// One level: the rows row0 .. row0 + n_rows of the panel's Sc simulations from the rows of their parents.  A unit is one simulation of
// one row; its LPS lanes are neighbours, lane p owns the pair of words p (the lanes p >= Wp only take part in the scan).  No lane
// leaves before the scan: a unit past the end computes nothing and stores nothing.  rows is read (earlier levels) and written (this
// level): no __restrict__.
template <int LPS>
__global__ void __launch_bounds__(256)
link_step_kernel(const int *__restrict__ fa_row, const int *__restrict__ mo_row, const long long *__restrict__ ids, int n_rows, long long row0,
                 ulonglong2 *rows, long long Cn, int Sc, int Wp, int W, int B, unsigned first_sim, unsigned q, unsigned k0, unsigned k1)
{
    constexpr int UPW = 64 / LPS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long u = (static_cast<long long>(blockIdx.x) * 4 + wave) * UPW + lane / LPS;
    const int p = lane % LPS;
    const bool mine = u < static_cast<long long>(n_rows) * Sc && p < Wp;
    const long long r = mine ? u / Sc : 0;
    const int s = mine ? static_cast<int>(u % Sc) : 0;
    const int parent[2] = {mine ? fa_row[r] : -1, mine ? mo_row[r] : -1};
    const u64 id = static_cast<u64>(ids[r]);
    const unsigned id_lo = static_cast<unsigned>(id), id_hi = static_cast<unsigned>(id >> 32);
    u64 X[2][2] = {{0, 0}, {0, 0}};
    unsigned odd = 0;                                    // bit side: this lane's two words hold an odd number of crossovers
#pragma unroll
    for (int side = 0; side < 2; ++side)
        if (parent[side] >= 0) {
            X[side][0] = genphi::link_crossover_word(id_lo, id_hi, first_sim + static_cast<unsigned>(s), side, 2 * p, q, k0, k1);
            if (2 * p + 1 < W) X[side][1] = genphi::link_crossover_word(id_lo, id_hi, first_sim + static_cast<unsigned>(s), side, 2 * p + 1, q, k0, k1);
            odd |= ((__popcll(X[side][0]) ^ __popcll(X[side][1])) & 1u) << side;
        }
    unsigned scan = odd;                                 // inclusive XOR scan over the unit's lanes
#pragma unroll
    for (int d = 1; d < LPS; d <<= 1) {
        const unsigned v = __shfl_up(scan, d, LPS);
        if (p >= d) scan ^= v;
    }
    const unsigned before = scan ^ odd;                  // the parity of all earlier words of the simulation
    const long long B2 = 2 * B;
    const long long c = static_cast<long long>(s) * Wp + p;
    ulonglong2 *dst = rows + ((row0 + r) * Cn + c) * B2;
#pragma unroll
    for (int side = 0; side < 2; ++side)
        if (parent[side] >= 0) {
            const u64 in0 = 0ull - ((before >> side) & 1u);
            const u64 t0 = genphi::link_prefix_xor(X[side][0]) ^ in0;
            const u64 in1 = 0ull - (t0 >> 63);
            const ulonglong2 T = make_ulonglong2(t0, genphi::link_prefix_xor(X[side][1]) ^ in1);
            const ulonglong2 *src = rows + (static_cast<long long>(parent[side]) * Cn + c) * B2;
            ulonglong2 *out = dst + side * B;
            for (int b = 0; b < B; ++b) {
                const ulonglong2 a = src[b], m = src[B + b];
                out[b] = meiosis(T, a, m);
            }
        }
}

// The 32 x 32 tile (blockIdx.y, blockIdx.x) of pairs over the Sc simulations of a panel (see the head of the file).  tile[]: word w
// of the pair, side, plane b, then 64 entries: the tile's 32 rows and its 32 columns.  Thread (ty, tx) owns the rows ty, ty + 16 and
// the columns tx, tx + 16.  sums[(i * n_pro + j) * 6 + k].
__global__ void __launch_bounds__(256)
link_pair_kernel(const ulonglong2 *__restrict__ gathered, int n_pro, int B, int Sc, int Wp, int L, int mirror, long long *__restrict__ sums)
{
    extern __shared__ u64 tile[];
    const int tr = blockIdx.y, tc = blockIdx.x;
    if (mirror && tr > tc) return;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int B2 = 2 * B;
    long long acc[2][2][6];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int v = 0; v < 6; ++v) acc[r][k][v] = 0;
    for (int s = 0; s < Sc; ++s) {
        int m[2][2] = {{0, 0}, {0, 0}}, n1[2][2] = {{0, 0}, {0, 0}}, n2[2][2] = {{0, 0}, {0, 0}}, g[2][2] = {{0, 0}, {0, 0}};
        u64 carry[2][2] = {{0, 0}, {0, 0}};
        for (int p = 0; p < Wp; ++p) {
            const long long col = static_cast<long long>(s) * Wp + p;
            __syncthreads();                             // the previous pair of words has been read
            for (int e = t; e < B2 * 64; e += 256) {
                const int idx = e & 63, k = e >> 6;
                const int gi = idx < LINK_TILE ? tr * LINK_TILE + idx : tc * LINK_TILE + idx - LINK_TILE;
                ulonglong2 v = make_ulonglong2(0, 0);
                if (gi < n_pro) v = gathered[(col * B2 + k) * n_pro + gi];
                tile[k * 64 + idx] = v.x;
                tile[(B2 + k) * 64 + idx] = v.y;
            }
            __syncthreads();
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const u64 mask = column_mask(L, 2 * p + w);
                if (mask == 0) continue;                 // (uniform) an odd W leaves the second word of the last pair empty
                const u64 *P = tile + w * B2 * 64, *M = P + B * 64;
                u64 nac[2][2] = {{0, 0}, {0, 0}}, nad[2][2] = {{0, 0}, {0, 0}}, nbc[2][2] = {{0, 0}, {0, 0}}, nbd[2][2] = {{0, 0}, {0, 0}};
                for (int b = 0; b < B; ++b) {
                    u64 a[2], bb[2], c[2], d[2];
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        a[r] = P[b * 64 + ty + 16 * r];
                        bb[r] = M[b * 64 + ty + 16 * r];
                        c[r] = P[b * 64 + LINK_TILE + tx + 16 * r];
                        d[r] = M[b * 64 + LINK_TILE + tx + 16 * r];
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
                        const u64 ac = ~nac[r][k] & mask, ad = ~nad[r][k] & mask, bc = ~nbc[r][k] & mask, bd = ~nbd[r][k] & mask;
                        const u64 any = ac | ad | bc | bd, two = (ac & bd) | (ad & bc);
                        m[r][k] += __popcll(ac) + __popcll(ad) + __popcll(bc) + __popcll(bd);
                        n1[r][k] += __popcll(any);
                        n2[r][k] += __popcll(two);
                        g[r][k] += __popcll(any & ~((any << 1) | carry[r][k]));
                        carry[r][k] = any >> 63;
                    }
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                long long *a = acc[r][k];
                a[0] += m[r][k];
                a[1] += static_cast<long long>(m[r][k]) * m[r][k];
                a[2] += n1[r][k];
                a[3] += n2[r][k];
                a[4] += g[r][k];
                a[5] += n1[r][k] > 0;
            }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = tr * LINK_TILE + ty + 16 * r, j = tc * LINK_TILE + tx + 16 * k;
            if (i >= n_pro || j >= n_pro) continue;
            long long *o = sums + (static_cast<long long>(i) * n_pro + j) * 6;
#pragma unroll
            for (int v = 0; v < 6; ++v) o[v] += acc[r][k][v];
            if (mirror && tr != tc) {                    // (j, i): all six sums are symmetric
                long long *o2 = sums + (static_cast<long long>(j) * n_pro + i) * 6;
#pragma unroll
                for (int v = 0; v < 6; ++v) o2[v] += acc[r][k][v];
            }
        }
}

// gen.simuSegments (include/genphi.h, genphi_seg_*): the lengths of the runs of `any`, on the tile, the staging and the ownership of
// link_pair_kernel, over the tiles with tile row <= tile column always.  Dynamic LDS: the tile (2048 * B bytes), then the workgroup's
// table (cells x 3 u64), then the edges.  Per word only the four inequality words, the masks and `any`; the walk (link_segments.h)
// carries a pair's open run from word to word of a simulation.  A closed run goes to the pair's counts of the simulation and, for
// i < j with both labels >= 0, to the table in LDS by 64-bit adds; the table goes to the global one once, its non-zero cells only, by
// 64-bit integer atomics (integer sums: the same bytes in any order).  pairs[(i * n_pro + j) * 3 + k]: one owner per pair and panel.
__global__ void __launch_bounds__(256)
link_segment_kernel(const ulonglong2 *__restrict__ gathered, int n_pro, int B, int Sc, int Wp, int L, const int *__restrict__ edges_in, int n_edges,
                    int min_loci, const int *__restrict__ group, int G, int cells, u64 *__restrict__ table_out, long long *__restrict__ pairs)
{
    extern __shared__ u64 tile[];
    const int tr = blockIdx.y, tc = blockIdx.x;
    if (tr > tc) return;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int B2 = 2 * B, W = (L + 63) >> 6;
    u64 *table = tile + 2 * B2 * 64;
    int *edges = reinterpret_cast<int *>(table + 3 * cells);
    for (int e = t; e < 3 * cells; e += 256) table[e] = 0;
    for (int e = t; e < n_edges; e += 256) edges[e] = edges_in[e];
    int cell0[2][2];                                     // the pair's first cell of the table, -1: the pair counts in no cell
    long long acc[2][2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = tr * LINK_TILE + ty + 16 * r, j = tc * LINK_TILE + tx + 16 * k;
            cell0[r][k] = -1;
            if (i < j && j < n_pro) {
                const int a = group[i], b = group[j];
                if (a >= 0 && b >= 0) cell0[r][k] = genphi::seg_group_pair(a, b, G) * (n_edges + 1);
            }
#pragma unroll
            for (int v = 0; v < 3; ++v) acc[r][k][v] = 0;
        }
    for (int s = 0; s < Sc; ++s) {
        genphi::SegState st[2][2];
        int over[2][2] = {{0, 0}, {0, 0}}, over_loci[2][2] = {{0, 0}, {0, 0}};
        for (int p = 0; p < Wp; ++p) {
            const long long col = static_cast<long long>(s) * Wp + p;
            __syncthreads();                             // the previous pair of words has been read (first: the table is zero)
            for (int e = t; e < B2 * 64; e += 256) {
                const int idx = e & 63, k = e >> 6;
                const int gi = idx < LINK_TILE ? tr * LINK_TILE + idx : tc * LINK_TILE + idx - LINK_TILE;
                ulonglong2 v = make_ulonglong2(0, 0);
                if (gi < n_pro) v = gathered[(col * B2 + k) * n_pro + gi];
                tile[k * 64 + idx] = v.x;
                tile[(B2 + k) * 64 + idx] = v.y;
            }
            __syncthreads();
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const u64 mask = column_mask(L, 2 * p + w);
                if (mask == 0) continue;                 // (uniform) an odd W leaves the second word of the last pair empty
                const int valid = min(64, L - 64 * (2 * p + w));
                const bool last = 2 * p + w == W - 1;
                const u64 *P = tile + w * B2 * 64, *M = P + B * 64;
                u64 nac[2][2] = {{0, 0}, {0, 0}}, nad[2][2] = {{0, 0}, {0, 0}}, nbc[2][2] = {{0, 0}, {0, 0}}, nbd[2][2] = {{0, 0}, {0, 0}};
                for (int b = 0; b < B; ++b) {
                    u64 a[2], bb[2], c[2], d[2];
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        a[r] = P[b * 64 + ty + 16 * r];
                        bb[r] = M[b * 64 + ty + 16 * r];
                        c[r] = P[b * 64 + LINK_TILE + tx + 16 * r];
                        d[r] = M[b * 64 + LINK_TILE + tx + 16 * r];
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
                        const u64 any = ~(nac[r][k] & nad[r][k] & nbc[r][k] & nbd[r][k]) & mask;
                        const int c0 = cell0[r][k];
                        int &n_over = over[r][k], &n_loci = over_loci[r][k];
                        genphi::seg_walk_word(any, valid, last, st[r][k], [&](int len, bool censored) {
                            if (len >= min_loci) {
                                n_over += 1;
                                n_loci += len;
                            }
                            if (c0 >= 0) {
                                u64 *cell = table + 3 * (c0 + genphi::seg_bin(edges, n_edges, len));
                                atomicAdd(cell, 1ull);
                                atomicAdd(cell + 1, static_cast<u64>(len));
                                if (censored) atomicAdd(cell + 2, 1ull);
                            }
                        });
                    }
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                acc[r][k][0] += over[r][k];
                acc[r][k][1] += over_loci[r][k];
                acc[r][k][2] += st[r][k].longest;
            }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = tr * LINK_TILE + ty + 16 * r, j = tc * LINK_TILE + tx + 16 * k;
            if (i >= n_pro || j >= n_pro) continue;
            long long *o = pairs + (static_cast<long long>(i) * n_pro + j) * 3;
#pragma unroll
            for (int v = 0; v < 3; ++v) o[v] += acc[r][k][v];
            if (tr != tc) {                              // (j, i): all three sums are symmetric
                long long *o2 = pairs + (static_cast<long long>(j) * n_pro + i) * 3;
#pragma unroll
                for (int v = 0; v < 3; ++v) o2[v] += acc[r][k][v];
            }
        }
    __syncthreads();                                     // every run of the workgroup is in the table
    for (int e = t; e < 3 * cells; e += 256) {
        const u64 v = table[e];
        if (v) atomicAdd(table_out + e, v);
    }
}

// labels[i][side][simulation][locus]: a lane per locus of a word, a wave per (proband, side, simulation, word); loci >= L are dropped.
__global__ void __launch_bounds__(256)
link_label_kernel(const ulonglong2 *__restrict__ gathered, int n_pro, int B, int Sc, int W, int Wp, int L, long long first_sim, long long S,
                  int *__restrict__ labels)
{
    const long long t = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const int bit = static_cast<int>(t & 63);
    const long long u = t >> 6;                          // ((proband * 2 + side) * Sc + simulation) * W + word
    if (u >= 2ll * n_pro * Sc * W) return;
    const int w = static_cast<int>(u % W);
    const long long v = u / W;
    const long long s = v % Sc, is = v / Sc;
    const int locus = 64 * w + bit;
    if (locus >= L) return;
    const ulonglong2 *src = gathered + (((s * Wp + (w >> 1)) * 2 + (is & 1)) * B) * n_pro + (is >> 1);
    int label = 0;
    for (int b = 0; b < B; ++b) {
        const ulonglong2 x = src[static_cast<long long>(b) * n_pro];
        label |= static_cast<int>(((w & 1 ? x.y : x.x) >> bit) & 1) << b;
    }
    labels[(is * S + first_sim + s) * L + locus] = label;
}

}  // namespace

struct genphi_link : LabelSweep {            // d_slots: the rows of one panel (n_live x simulations x Wp pairs x 2 sides x B planes x 16 bytes)
    genphi::LinkShape shape;                 // L, q, W, Wp, the lanes per simulation (link.h)
    bool want_labels = false, all_pairs = false;
    DevBuf<long long> d_sums;
    DevBuf<int> d_labels;
    DevBuf<ulonglong2> d_gathered;           // the listed probands' rows of one panel, transposed (label_gather_kernel)
    int64_t sims = 0;                        // simulations of a panel
    int64_t n_panels = 0;
    double pair_ms = 0.0, word_ops = 0.0, philox_blocks = 0.0;
    // gen.simuSegments (genphi_seg_*): the request that the next compute answers, and the one that the last compute answered
    struct SegRequest {
        std::vector<int32_t> edges, group;   // no edges: no request; group: a label per list position (zeros without groups)
        int32_t min_loci = 1, n_groups = 0;
        int32_t n_edges() const { return static_cast<int32_t>(edges.size()); }
        int32_t G() const { return n_groups > 1 ? n_groups : 1; }
    } seg_next, seg_ran;
    DevBuf<u64> d_seg_table;                 // cells x 3, the pairs of groups a <= b (link_segments.h)
    DevBuf<long long> d_seg_pairs;           // n_pro x n_pro x 3
    DevBuf<int> d_seg_lists;                 // the edges, then the labels
    double seg_ms = 0.0, seg_word_ops = 0.0;
    int64_t seg_lds = 0, seg_closed = 0;     // the segments closed: the sum of the table's first counters
    genphi_link() { own(d_sums, d_labels, d_gathered, d_seg_table, d_seg_pairs, d_seg_lists); }
};

namespace {

// the simulations of a panel: panel_arg cut to S, 0 = all of S (drop_plan.h counts in units of 128 columns: a simulation is one unit)
int64_t panel_sims(int64_t S, int32_t panel_arg) { return genphi::drop_panel_pairs(128 * S, 128 * static_cast<int64_t>(panel_arg)); }

// The panel width, the rows, the results and the lists on the device; GENPHI_ERR_ALLOC before any launch.
int prepare(genphi_link *h)
{
    const genphi::IdentPlan &pl = h->plan;
    const genphi::LinkSizes z = genphi::link_sizes(pl, h->S, h->shape, h->want_labels);
    double usable = 0.0;
    if (int rc = h->usable_bytes(usable, h->held_bytes())) return rc;
    const genphi::SegSizes zs = genphi::seg_sizes(pl.n_pro, h->seg_next.n_edges(), h->seg_next.n_groups);
    const double room = usable - static_cast<double>(z.fixed()) - static_cast<double>(zs.fixed()) - (64 << 20);
    const double sim_bytes = static_cast<double>(z.panel(1));
    int64_t Sn;
    if (!genphi::drop_panel_fits(Sn, 128 * h->S, 128 * static_cast<int64_t>(h->panel_arg), room, sim_bytes))
        return genphi_set_error(GENPHI_ERR_ALLOC, "gen.simuSharing: the sums of " + std::to_string(pl.n_pro) + " probands" +
                                                      (h->want_labels ? ", the labels" : "") + (zs.fixed() ? ", the segment tables" : "") + " and " + std::to_string(pl.n_live) + " live rows of " +
                                                      std::to_string(pl.planes) + " planes, " + std::to_string(h->shape.L) + " loci and " +
                                                      std::to_string(std::max<int64_t>(Sn, 1)) + " simulations do not fit on device " + std::to_string(h->device));
    GENPHI_HIP_TRY(h->d_slots.reserve(z.sim_rows * static_cast<size_t>(Sn)));
    GENPHI_HIP_TRY(h->d_gathered.reserve(z.sim_gather * static_cast<size_t>(Sn) / sizeof(ulonglong2)));
    GENPHI_HIP_TRY(h->d_sums.reserve(z.sums / 8));
    if (h->want_labels) GENPHI_HIP_TRY(h->d_labels.reserve(z.labels / 4));
    if (zs.fixed()) {
        GENPHI_HIP_TRY(h->d_seg_table.reserve(zs.table / 8));
        GENPHI_HIP_TRY(h->d_seg_pairs.reserve(zs.pairs / 8));
        GENPHI_HIP_TRY(h->d_seg_lists.reserve((zs.edges + zs.labels) / 4));
    }
    if (int rc = h->upload_lists()) return rc;
    h->sims = Sn;
    h->n_panels = (h->S + Sn - 1) / Sn;
    return GENPHI_OK;
}

// the step kernel's form for LPS lanes per simulation (link_shape: a power of two, at most 32)
#define LINK_STEP_CASE(LPS)                                                                                                                       \
    case LPS:                                                                                                                                     \
        link_step_kernel<LPS><<<grid, 256, 0, h->stream>>>(h->d_fa.get() + b, h->d_mo.get() + b, h->d_ids.get() + b, n_rows, b, rows, Cn, Sc, Wp, \
                                                           sh.W, B, static_cast<unsigned>(s0), static_cast<unsigned>(sh.q), k0, k1);            \
        break

int compute_impl(genphi_link *h, int32_t device)
{
    if (int rc = h->select(device)) return rc;           // (computed = false: a compute that fails leaves no result, segments included)
    h->seg_ran = genphi_link::SegRequest();              // before prepare() may replace the blocks of the request answered last
    if (int rc = prepare(h)) return rc;
    const genphi::IdentPlan &pl = h->plan;
    const genphi::LinkShape &sh = h->shape;
    const int lps = sh.lanes, B = pl.planes, n_pro = static_cast<int>(pl.n_pro), Wp = sh.Wp;
    const int64_t Sn = h->sims;
    const long long Cn = static_cast<long long>(Sn) * Wp;
    const unsigned k0 = static_cast<unsigned>(h->seed), k1 = static_cast<unsigned>(h->seed >> 32);
    ulonglong2 *rows = h->slots<ulonglong2>();
    const int step_units = 4 * (64 / lps);
    const unsigned tiles = static_cast<unsigned>((n_pro + LINK_TILE - 1) / LINK_TILE);
    const size_t lds = static_cast<size_t>(2 * 2 * 64 * 8) * static_cast<size_t>(B);
    PhaseTimer timer, seg_timer;
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_sums.get(), 0, h->d_sums.bytes(), h->stream));
    // gen.simuSegments: the request as it stands now is the one this compute answers
    const genphi_link::SegRequest &rq = h->seg_next;
    const genphi::SegSizes zs = genphi::seg_sizes(n_pro, rq.n_edges(), rq.n_groups);
    const int seg_cells = rq.n_edges() ? static_cast<int>(genphi::seg_cells(rq.n_edges(), rq.n_groups)) : 0;
    const size_t seg_lds = rq.n_edges() ? genphi::seg_lds_bytes(B, rq.n_edges(), rq.n_groups) : 0;
    if (rq.n_edges()) {
        GENPHI_HIP_TRY(hipMemsetAsync(h->d_seg_table.get(), 0, zs.table, h->stream));
        GENPHI_HIP_TRY(hipMemsetAsync(h->d_seg_pairs.get(), 0, zs.pairs, h->stream));
        GENPHI_HIP_TRY(hipMemcpyAsync(h->d_seg_lists.get(), rq.edges.data(), zs.edges, hipMemcpyHostToDevice, h->stream));
        GENPHI_HIP_TRY(hipMemcpyAsync(h->d_seg_lists.get() + rq.n_edges(), rq.group.data(), zs.labels, hipMemcpyHostToDevice, h->stream));
        GENPHI_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(link_segment_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           static_cast<int>(seg_lds)));
    }
    double seg_ms = 0.0, seg_idle = 0.0;                 // seg_idle: the empty first phase of seg_timer, never reported
    double sweep_ms = 0.0, pair_ms = 0.0;
    int64_t launches = 0;
    for (int64_t s0 = 0; s0 < h->S; s0 += Sn) {
        const int Sc = static_cast<int>(std::min<int64_t>(Sn, h->S - s0));
        const long long Cc = static_cast<long long>(Sc) * Wp;
        if (int rc = timer.begin(h->stream)) return rc;
        if (int rc = h->init_panel(Cn, Cc)) return rc;
        for (int k = 1; k < pl.n_levels; ++k) {
            const long long b = pl.level_begin[k];
            const int n_rows = static_cast<int>(pl.level_rows[k]);
            const long long units = static_cast<long long>(n_rows) * Sc;
            const unsigned grid = static_cast<unsigned>((units + step_units - 1) / step_units);
            switch (lps) {
                LINK_STEP_CASE(1);
                LINK_STEP_CASE(2);
                LINK_STEP_CASE(4);
                LINK_STEP_CASE(8);
                LINK_STEP_CASE(16);
                LINK_STEP_CASE(32);
            default: return genphi_set_error(GENPHI_ERR_ARG, "gen.simuSharing: " + std::to_string(lps) + " lanes per simulation");
            }
            GENPHI_HIP_TRY(hipGetLastError());
        }
        if (int rc = timer.middle(h->stream)) return rc;
        if (int rc = h->gather_panel(Cn, Cc, h->d_gathered.get())) return rc;
        link_pair_kernel<<<dim3(tiles, tiles), 256, lds, h->stream>>>(h->d_gathered.get(), n_pro, B, Sc, Wp, sh.L, h->all_pairs ? 0 : 1, h->d_sums.get());
        GENPHI_HIP_TRY(hipGetLastError());
        if (int rc = timer.end(h->stream)) return rc;
        if (rq.n_edges()) {
            // the kernel alone between two events: PhaseTimer's first phase (begin .. middle) is empty here, its second is segment_ms
            if (int rc = seg_timer.begin(h->stream)) return rc;
            if (int rc = seg_timer.middle(h->stream)) return rc;
            link_segment_kernel<<<dim3(tiles, tiles), 256, seg_lds, h->stream>>>(h->d_gathered.get(), n_pro, B, Sc, Wp, sh.L, h->d_seg_lists.get(), rq.n_edges(),
                                                                                 rq.min_loci, h->d_seg_lists.get() + rq.n_edges(), rq.G(), seg_cells,
                                                                                 h->d_seg_table.get(), h->d_seg_pairs.get());
            GENPHI_HIP_TRY(hipGetLastError());
            if (int rc = seg_timer.end(h->stream)) return rc;
        }
        if (h->want_labels) {
            const long long threads = 2ll * n_pro * Sc * sh.W * 64;
            link_label_kernel<<<static_cast<unsigned>((threads + 255) / 256), 256, 0, h->stream>>>(h->d_gathered.get(), n_pro, B, Sc, sh.W, Wp, sh.L, s0, h->S,
                                                                                                   h->d_labels.get());
            GENPHI_HIP_TRY(hipGetLastError());
        }
        if (int rc = timer.add(sweep_ms, pair_ms)) return rc;
        if (rq.n_edges())
            if (int rc = seg_timer.add(seg_idle, seg_ms)) return rc;
        launches += pl.n_levels + 2 + (h->want_labels ? 1 : 0) + (rq.n_edges() ? 1 : 0);
    }
    GENPHI_HIP_TRY(hipStreamSynchronize(h->stream));
    // per side with a known parent and simulation: two runs of B planes read and one written, 16 bytes per plane and pair of words
    const double known_sides = 2.0 * static_cast<double>(pl.n_live) - static_cast<double>(pl.n_labels);
    const double n = static_cast<double>(n_pro), S = static_cast<double>(h->S);
    h->sweep_ms = sweep_ms;
    h->pair_ms = pair_ms;
    h->alg_bytes = 3.0 * 16.0 * B * known_sides * S * Wp;
    h->word_ops = (h->all_pairs ? n * n : n * (n + 1.0) / 2.0) * S * sh.W * (8.0 * B + 32.0);
    h->philox_blocks = known_sides * S * static_cast<double>(genphi::link_blocks_per_side(sh));
    h->n_launches = launches;
    h->seg_closed = 0;
    if (rq.n_edges()) {                                  // the segments closed, read from the table (at most 48 KB)
        std::vector<int64_t> upper(zs.table / 8);
        if (int rc = h->copy_out(upper.data(), h->d_seg_table.get(), zs.table, "gen.simuSegments")) return rc;
        for (size_t c = 0; c < upper.size(); c += 3) h->seg_closed += upper[c];
    }
    h->seg_ran = rq;
    h->seg_ms = seg_ms;
    h->seg_word_ops = rq.n_edges() ? n * (n + 1.0) / 2.0 * S * sh.W * (8.0 * B + 10.0) : 0.0;
    h->seg_lds = static_cast<int64_t>(seg_lds);
    h->computed = true;
    return GENPHI_OK;
}

}  // namespace

extern "C" {

int genphi_link_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro, const int64_t *pro_ids,
                       int32_t loci, int32_t q, int64_t simul_no, uint64_t seed, int32_t panel_sims_arg, int32_t flags, genphi_link **out)
{
    if (out) *out = nullptr;
    if (out && (flags & ~(GENPHI_LINK_FLAG_LABELS | GENPHI_LINK_FLAG_ALL_PAIRS))) return genphi_set_error(GENPHI_ERR_ARG, "genphi_link_create: unknown flag");
    if (int rc = check_create_args("genphi_link_create", n_ind, ind, father, mother, n_pro, pro_ids, 0, nullptr, out, 0)) return rc;
    if (n_pro == 0) return genphi_set_error(GENPHI_ERR_ARG, "gen.simuSharing: no probands");
    if (n_pro * n_pro >= (int64_t(1) << 31))
        return genphi_set_error(GENPHI_ERR_ARG, "gen.simuSharing: " + std::to_string(n_pro) + " probands: 2^31 or more ordered pairs");
    if (simul_no < 1 || simul_no > GENPHI_SIMU_MAX_SIMULATIONS)
        return genphi_set_error(GENPHI_ERR_ARG, "gen.simuSharing: simulNo = " + std::to_string(simul_no) + " is outside 1 .. 2^24");
    if (loci < 1 || loci > genphi::kLinkMaxLoci) return genphi_set_error(GENPHI_ERR_ARG, "gen.simuSharing: loci = " + std::to_string(loci) + " is outside 1 .. 4096");
    if (q < 0 || q > genphi::kLinkMaxQ) return genphi_set_error(GENPHI_ERR_ARG, "gen.simuSharing: q = " + std::to_string(q) + " is outside 0 .. 32768");
    if (panel_sims_arg < 0) return genphi_set_error(GENPHI_ERR_ARG, "genphi_link_create: panel_sims is 0 (the default rule) or positive");
    return create_entry(out, "gen.simuSharing", [&](genphi_link *h) {
        h->S = simul_no;
        h->seed = seed;
        h->shape = genphi::link_shape(loci, q);
        h->want_labels = (flags & GENPHI_LINK_FLAG_LABELS) != 0;
        h->all_pairs = (flags & GENPHI_LINK_FLAG_ALL_PAIRS) != 0;
        h->panel_arg = panel_sims_arg;
        std::string err;
        if (const int rc = genphi::plan_ident(h->plan, n_ind, ind, father, mother, n_pro, pro_ids, err)) return genphi_set_error(rc, err);
        // labels no device memory can hold are refused here, on the host; what a given device holds is known at compute
        if (h->want_labels && static_cast<double>(genphi::link_sizes(h->plan, simul_no, h->shape, true).labels) >= 281474976710656.0)
            return genphi_set_error(GENPHI_ERR_ALLOC, "gen.simuSharing: the labels of " + std::to_string(n_pro) + " probands, " + std::to_string(simul_no) +
                                                          " simulations and " + std::to_string(loci) + " loci are 2^48 bytes or more");
        h->sims = panel_sims(simul_no, panel_sims_arg);       // (compute may narrow the default to what fits)
        h->n_panels = (simul_no + h->sims - 1) / h->sims;
        return GENPHI_OK;
    });
}

int genphi_link_levels(const genphi_link *h, int64_t *n_live, int32_t *levels, int64_t *rows_per_level)
{
    return drop_levels(h, "genphi_link_levels", n_live, levels, rows_per_level);
}

int genphi_link_alleles(const genphi_link *h, int64_t *n_labels, int32_t *planes, int64_t *ids, int32_t *sides)
{
    return label_alleles(h, "genphi_link_alleles", n_labels, planes, ids, sides);
}

int genphi_link_compute(genphi_link *h, int32_t device) { return compute_entry(h, device, "genphi_link_compute", "gen.simuSharing", compute_impl); }

int genphi_link_sums_to_host(genphi_link *h, int64_t *out)
{
    return result_to_host(h, out, &genphi_link::d_sums, "genphi_link_sums_to_host", "gen.simuSharing");
}

int genphi_link_labels_to_host(genphi_link *h, int32_t *out)
{
    return labels_to_host(h, out, "genphi_link_labels_to_host", "GENPHI_LINK_FLAG_LABELS", "gen.simuSharing");
}

int genphi_link_stats(const genphi_link *h, double *sweep_ms, double *pair_ms, double *algorithmic_bytes, double *word_ops, double *philox_blocks,
                      int32_t *levels, int32_t *panel_sims_out, int64_t *panels, int32_t *planes, int32_t *tile_rows, int32_t *tile_cols,
                      int32_t *lanes_per_sim)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_link_stats: NULL handle");
    h->stats(sweep_ms, algorithmic_bytes, nullptr);
    put(pair_ms, h->pair_ms);
    put(word_ops, h->word_ops);
    put(philox_blocks, h->philox_blocks);
    put(levels, h->plan.n_levels);
    put(panel_sims_out, h->sims);
    put(panels, h->n_panels);
    put(planes, h->plan.planes);
    put(tile_rows, LINK_TILE);
    put(tile_cols, LINK_TILE);
    put(lanes_per_sim, h->shape.lanes);
    return GENPHI_OK;
}

void genphi_link_destroy(genphi_link *h) { destroy_entry(h); }

int genphi_seg_request(genphi_link *h, int32_t n_edges, const int32_t *edges, int32_t min_loci, int32_t n_groups, const int32_t *group)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_seg_request: NULL handle");
    if (n_edges == 0) {
        h->seg_next = genphi_link::SegRequest();
        return GENPHI_OK;
    }
    const int64_t n_pro = h->plan.n_pro;
    const std::string err = genphi::seg_check_request(n_edges, edges, min_loci, n_groups, group, n_pro);
    if (!err.empty()) return genphi_set_error(GENPHI_ERR_ARG, "gen.simuSegments: " + err);
    try {
        genphi_link::SegRequest rq;
        rq.edges.assign(edges, edges + n_edges);
        if (n_groups > 0) rq.group.assign(group, group + n_pro);
        else rq.group.assign(static_cast<size_t>(n_pro), 0);
        rq.min_loci = min_loci;
        rq.n_groups = n_groups;
        h->seg_next = std::move(rq);
    } catch (const std::bad_alloc &) { return genphi_set_error(GENPHI_ERR_ALLOC, "out of host memory in gen.simuSegments"); }
    return GENPHI_OK;
}

int genphi_seg_to_host(genphi_link *h, int64_t *hist, int64_t *pairs)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_seg_to_host: nothing computed");
    const genphi_link::SegRequest &rq = h->seg_ran;
    if (!rq.n_edges()) return genphi_set_error(GENPHI_ERR_ARG, "genphi_seg_to_host: the last compute ran without a request (genphi_seg_request)");
    const genphi::SegSizes zs = genphi::seg_sizes(h->plan.n_pro, rq.n_edges(), rq.n_groups);
    if (pairs)
        if (int rc = h->copy_out(pairs, h->d_seg_pairs.get(), zs.pairs, "gen.simuSegments")) return rc;
    if (hist) {
        try {
            std::vector<int64_t> upper(zs.table / 8);
            if (int rc = h->copy_out(upper.data(), h->d_seg_table.get(), zs.table, "gen.simuSegments")) return rc;
            const int32_t G = rq.G();
            const size_t row = 3 * static_cast<size_t>(rq.n_edges() + 1);                // the Int64 of one pair of groups
            for (int32_t a = 0; a < G; ++a)
                for (int32_t b = 0; b < G; ++b)
                    std::copy_n(upper.data() + row * static_cast<size_t>(genphi::seg_group_pair(a, b, G)), row, hist + row * (static_cast<size_t>(a) * G + b));
        } catch (const std::bad_alloc &) { return genphi_set_error(GENPHI_ERR_ALLOC, "out of host memory in gen.simuSegments"); }
    }
    return GENPHI_OK;
}

int genphi_seg_stats(const genphi_link *h, double *segment_ms, double *word_ops, int64_t *segments, int32_t *cells, int64_t *lds_bytes)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_seg_stats: NULL handle");
    const genphi_link::SegRequest &rq = h->seg_ran;
    const bool ran = h->computed && rq.n_edges();
    const int64_t n_cells = ran ? genphi::seg_cells(rq.n_edges(), rq.n_groups) : 0;
    put(segment_ms, ran ? h->seg_ms : 0.0);
    put(word_ops, ran ? h->seg_word_ops : 0.0);
    put(segments, ran ? h->seg_closed : int64_t(0));
    put(cells, n_cells);
    put(lds_bytes, ran ? h->seg_lds : int64_t(0));
    return GENPHI_OK;
}

}  // extern "C"
