// simu.hip -- gen.simuSample / gen.simuProb: gene dropping (include/genphi.h, genphi_simu_*).
//
// GENLIB's gen.simuSample and gen.simuProb (the reference has no form of them; the definition is the text in include/genphi.h):
// marked alleles of chosen ancestors are dropped down the pedigree S times and counted in the probands.  A simulation needs one
// bit per parental side and individual, so 64 simulations share a word: every individual x has two bit rows over the simulations,
// P_x (the copy from its father is marked) and M_x, and a meiosis is (T & P_parent) | (~T & M_parent) with a random word T.
//
// Here: a level-synchronous sweep, top-down.  The host plan (simu.h, no GPU) lists the live set L by level; rows of the device
// buffer are positions in L.
//   layout  a panel row holds Pn 16-byte pairs of words per side; the P pair and the M pair of one individual and pair index are
//           neighbours: row r, pair j = 32 bytes at ((r * Pn + j) * 2) ulonglong2: {P[2j], P[2j + 1]}, {M[2j], M[2j + 1]}
//   init    the rows of level 0 from the states of the listed ancestors (all ones / zero).  Only these rows are ever
//           initialised: every other row is fully written by its own step before anything reads it
//   step    one launch per level >= 1: LPR lanes per row (a power of two), a lane owns one pair: it loads the 32 bytes of each
//           live parent, draws one Philox4x32-10 block per side (two 64-bit words = one pair) keyed on (seed, ID, side, ABSOLUTE
//           pair index) and stores its 32 bytes.  Parents come from any earlier level: all rows of a panel stay resident
//   states  per listed proband (a wave each) and panel: popcounts of P & M, P ^ M and ~(P | M), masked to the columns < S,
//           added into the Int64 table (n_pro, 3); the panels of a sweep run one after the other on one stream: plain adds
//   sample  on request: the bits expanded into the Int8 matrix (n_pro, S); a lane expands whole words (4 columns per 32-bit
//           multiply), 16-byte stores where S is a multiple of 16
//   match   gen.simuProb: per simulation column, the listed probands whose count equals statePro[i]: the bit-plane column count
//           of implex_count_kernel (a lane owns a word and walks at most 255 probands per plane set), Int32 atomics
// Everything is integer and keyed on IDs and absolute word indices: the same bits on every run, with any panel width.
#include <hip/hip_runtime.h>

#include "drop_device.h"
#include "drop_host.h"
#include "simu.h"

namespace {

// Level 0: a thread per (row, pair).  State 1: P = all ones, M = 0; state 2: both all ones (columns >= S are never counted).
__global__ void __launch_bounds__(256)
simu_init_kernel(const int *__restrict__ state0, long long n_rows, ulonglong2 *__restrict__ rows, int Pn, int Pc)
{
    const long long t = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const long long row = t / Pc;
    if (row >= n_rows) return;
    const int c = static_cast<int>(t % Pc);
    const u64 m = state0[row] == 2 ? ~0ull : 0ull;
    ulonglong2 *dst = rows + (row * Pn + c) * 2;
    dst[0] = make_ulonglong2(~0ull, ~0ull);
    dst[1] = make_ulonglong2(m, m);
}

// One level: row row0 + r from the rows of its parents.  LPR lanes per row, lane l owns the pairs l, l + LPR, .. < Pc of a row
// of Pn pairs; a wave holds 64 / LPR rows.  rows is read (earlier levels) and written (this level): no __restrict__.
template <int LPR>
__global__ void __launch_bounds__(256)
simu_step_kernel(const int *__restrict__ fa_row, const int *__restrict__ mo_row, const long long *__restrict__ ids, int n_rows,
                 long long row0, ulonglong2 *rows, int Pn, int Pc, unsigned first_pair, unsigned k0, unsigned k1)
{
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = (static_cast<long long>(blockIdx.x) * 4 + wave) * RPW + lane / LPR;
    if (r >= n_rows) return;
    const int l = lane % LPR;
    const int f = fa_row[r], m = mo_row[r];
    const u64 id = static_cast<u64>(ids[r]);
    const unsigned id_lo = static_cast<unsigned>(id), id_hi = static_cast<unsigned>(id >> 32);
    const ulonglong2 *fs = rows + static_cast<long long>(f < 0 ? 0 : f) * Pn * 2;
    const ulonglong2 *ms = rows + static_cast<long long>(m < 0 ? 0 : m) * Pn * 2;
    ulonglong2 *dst = rows + (row0 + r) * Pn * 2;
    for (int c = l; c < Pc; c += LPR) {
        ulonglong2 px = make_ulonglong2(0, 0), mx = make_ulonglong2(0, 0);
        if (f >= 0) {
            const ulonglong2 a = fs[2 * c], b = fs[2 * c + 1];
            const ulonglong2 T = philox_pair(id_lo, id_hi, first_pair + static_cast<unsigned>(c), 0u, k0, k1);
            px = meiosis(T, a, b);
        }
        if (m >= 0) {
            const ulonglong2 a = ms[2 * c], b = ms[2 * c + 1];
            const ulonglong2 T = philox_pair(id_lo, id_hi, first_pair + static_cast<unsigned>(c), 1u, k0, k1);
            mx = meiosis(T, a, b);
        }
        dst[2 * c] = px;
        dst[2 * c + 1] = mx;
    }
}

// A wave per listed proband: the columns of the panel with 0, 1 and 2 copies, added to counts[i][0..2].
__global__ void __launch_bounds__(256)
simu_states_kernel(const ulonglong2 *__restrict__ rows, const int *__restrict__ pro_row, long long n_pro, int Pn, int Pc,
                   unsigned first_pair, long long S, long long *__restrict__ counts)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i = static_cast<long long>(blockIdx.x) * 4 + wave;
    if (i >= n_pro) return;
    const int r = pro_row[i];
    const ulonglong2 *src = rows + static_cast<long long>(r < 0 ? 0 : r) * Pn * 2;
    int n1 = 0, n2 = 0, nv = 0;
    for (int c = lane; c < Pc; c += 64) {
        ulonglong2 p = make_ulonglong2(0, 0), m = make_ulonglong2(0, 0);
        if (r >= 0) { p = src[2 * c]; m = src[2 * c + 1]; }
        const long long w = 2 * (static_cast<long long>(first_pair) + c);
        const u64 k0 = column_mask(S, w), k1 = column_mask(S, w + 1);
        n2 += __popcll(p.x & m.x & k0) + __popcll(p.y & m.y & k1);
        n1 += __popcll((p.x ^ m.x) & k0) + __popcll((p.y ^ m.y) & k1);
        nv += __popcll(k0) + __popcll(k1);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        n1 += __shfl_xor(n1, d, 64);
        n2 += __shfl_xor(n2, d, 64);
        nv += __shfl_xor(nv, d, 64);
    }
    if (lane == 0) {
        counts[i * 3] += nv - n1 - n2;
        counts[i * 3 + 1] += n1;
        counts[i * 3 + 2] += n2;
    }
}

// four bits -> four bytes (bit k in byte k): the four shifted copies do not overlap, so the multiply carries nothing
__device__ __forceinline__ unsigned spread4(unsigned nibble) { return (nibble * 0x00204081u) & 0x01010101u; }

// The Int8 matrix (n_pro, S), row-major: a thread per (proband, word of the panel) expands its 64 columns.
__global__ void __launch_bounds__(256)
simu_sample_kernel(const u64 *__restrict__ rows, const int *__restrict__ pro_row, long long n_pro, int Pn, int Wc, long long first_word,
                   long long S, signed char *__restrict__ sample)
{
    const long long t = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const long long i = t / Wc;
    if (i >= n_pro) return;
    const int w = static_cast<int>(t % Wc);
    const long long col0 = 64 * (first_word + w), left = S - col0;
    if (left <= 0) return;
    const int r = pro_row[i];
    u64 p = 0, m = 0;
    if (r >= 0) {
        const long long base = (static_cast<long long>(r) * Pn + (w >> 1)) * 4 + (w & 1);
        p = rows[base];
        m = rows[base + 2];
    }
    signed char *out = sample + i * S + col0;
    if (left >= 64 && (S & 15) == 0) {                   // rows start on 16 bytes
        uint4 *o = reinterpret_cast<uint4 *>(out);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned pq = static_cast<unsigned>(p >> (16 * q)) & 0xFFFFu, mq = static_cast<unsigned>(m >> (16 * q)) & 0xFFFFu;
            uint4 v;
            v.x = spread4(pq & 15) + spread4(mq & 15);
            v.y = spread4((pq >> 4) & 15) + spread4((mq >> 4) & 15);
            v.z = spread4((pq >> 8) & 15) + spread4((mq >> 8) & 15);
            v.w = spread4(pq >> 12) + spread4(mq >> 12);
            o[q] = v;
        }
    } else {
        const int n = static_cast<int>(left < 64 ? left : 64);
        for (int b = 0; b < n; ++b) out[b] = static_cast<signed char>(((p >> b) & 1) + ((m >> b) & 1));
    }
}

// Per simulation column, the listed probands whose count equals state_pro[i].  LPR lanes per row means LPR WORDS (a power of
// two): lane l of a group owns word blockIdx.y * LPR + l of the probands its group walks, 256 / LPR groups per block, block x owns
// SIMU_MATCH_ROWS * 256 / LPR consecutive probands and deals them round-robin to its groups, so a group walks at most 255
// probands: eight bit planes hold the count of every bit (implex_count_kernel).
constexpr int SIMU_MATCH_ROWS = 255;

template <int LPR>
__global__ void __launch_bounds__(256)
simu_match_kernel(const u64 *__restrict__ rows, const int *__restrict__ pro_row, const int *__restrict__ state_pro, long long n_pro,
                  int Pn, int Wc, long long first_word, long long S, unsigned *__restrict__ match)
{
    constexpr int GPB = 256 / LPR;
    __shared__ unsigned sums[LPR * 64];
    for (int i = threadIdx.x; i < LPR * 64; i += 256) sums[i] = 0;
    __syncthreads();
    const int grp = threadIdx.x / LPR, l = threadIdx.x % LPR;
    const int w = static_cast<int>(blockIdx.y) * LPR + l;
    const long long r0 = static_cast<long long>(blockIdx.x) * (GPB * SIMU_MATCH_ROWS);
    const long long r1 = min(r0 + GPB * SIMU_MATCH_ROWS, n_pro);
    if (w < Wc && r0 + grp < r1) {
        u64 plane[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) plane[k] = 0;
        for (long long i = r0 + grp; i < r1; i += GPB) {
            const int r = pro_row[i], st = state_pro[i];
            u64 p = 0, m = 0;
            if (r >= 0) {
                const long long base = (static_cast<long long>(r) * Pn + (w >> 1)) * 4 + (w & 1);
                p = rows[base];
                m = rows[base + 2];
            }
            u64 carry = st == 2 ? (p & m) : (st == 1 ? (p ^ m) : ~(p | m));
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
        const int wl = static_cast<int>(blockIdx.y) * LPR + i / 64;
        const long long col = 64 * (first_word + wl) + (i & 63);
        if (v && wl < Wc && col < S) atomicAdd(&match[col], v);
    }
}

}  // namespace

struct genphi_simu : SweepDevice {           // d_slots: the rows of one panel (2 x n_live x pairs x 16 bytes)
    genphi::SimuPlan plan;                   // host plan (simu.h)
    int64_t S = 0;
    uint64_t seed = 0;
    bool no_sample = false;
    int32_t panel_env = 0;                   // GENPHI_SIMU_PANEL (0 = default rule)
    DevBuf<long long> d_counts;              // n_pro x 3
    DevBuf<signed char> d_sample;            // n_pro x S, unless no_sample
    DevBuf<unsigned> d_match;                // S
    DevBuf<int> d_state_pro;                 // n_pro, the states of the last match_counts
    DevBuf<int> d_fa, d_mo, d_state0, d_pro_row;
    DevBuf<long long> d_ids;
    DropPanels panels;
    genphi_simu() { own(d_counts, d_sample, d_match, d_state_pro, d_fa, d_mo, d_state0, d_pro_row, d_ids); }
    bool empty() const { return false; }     // (n_pro >= 1 and S >= 1 always)
    size_t sample_bytes() const { return no_sample ? 0 : static_cast<size_t>(plan.n_pro) * static_cast<size_t>(S); }
};

namespace {

// The panel width, the rows and the lists on the device; GENPHI_ERR_ALLOC before any launch.
int prepare(genphi_simu *h, int32_t device)
{
    const genphi::SimuPlan &pl = h->plan;
    const size_t n_pro = static_cast<size_t>(pl.n_pro);
    const size_t res_bytes = 24 * n_pro + h->sample_bytes() + 4 * static_cast<size_t>(h->S) + 4 * n_pro;
    double usable = 0.0;
    if (int rc = h->usable_bytes(usable, h->d_counts.get() ? res_bytes : 0)) return rc;
    const double list_bytes = 4.0 * static_cast<double>(pl.fa_row.size() + pl.mo_row.size() + pl.state0.size() + pl.pro_row.size()) +
                              8.0 * static_cast<double>(pl.row_id.size());
    const double room = usable - static_cast<double>(res_bytes) - (h->d_pro_row.get() ? 0.0 : list_bytes) - (64 << 20);
    const double pair_bytes = 32.0 * static_cast<double>(pl.n_live);                   // one pair of every row, both sides
    int64_t Pn;
    if (!genphi::drop_panel_fits(Pn, h->S, h->panel_env, room, pair_bytes))
        return genphi_set_error(GENPHI_ERR_ALLOC, "gen.simu: " + std::to_string(pl.n_live) + " live rows of " + std::to_string(128 * std::max<int64_t>(Pn, 1)) +
                                                      " simulations do not fit on device " + std::to_string(device) + " beside the results");
    GENPHI_HIP_TRY(h->d_slots.reserve(static_cast<size_t>(pl.n_live) * static_cast<size_t>(Pn) * 32));
    GENPHI_HIP_TRY(h->d_counts.reserve(3 * n_pro));
    if (!h->no_sample) GENPHI_HIP_TRY(h->d_sample.reserve(h->sample_bytes()));
    GENPHI_HIP_TRY(h->d_match.reserve(static_cast<size_t>(h->S)));
    GENPHI_HIP_TRY(h->d_state_pro.reserve(n_pro));
    int rc;
    if ((rc = h->upload(h->d_fa, pl.fa_row)) || (rc = h->upload(h->d_mo, pl.mo_row)) || (rc = h->upload(h->d_state0, pl.state0)) ||
        (rc = h->upload(h->d_pro_row, pl.pro_row)) || (rc = h->upload(h->d_ids, pl.row_id)))
        return rc;
    h->panels.set(h->S, Pn);
    return GENPHI_OK;
}

// The panels, one after the other on the handle's stream.  sweep: init and the level steps of every panel (else: the resident rows
// of the single panel are read); results: state counts and sample; match: the match counts for d_state_pro.
int run_panels(genphi_simu *h, bool sweep, bool results, bool match)
{
    const genphi::SimuPlan &pl = h->plan;
    const int Pn = h->panels.pairs, lpr = h->panels.lanes_per_row;
    const int64_t total = h->panels.total;
    const unsigned k0 = static_cast<unsigned>(h->seed), k1 = static_cast<unsigned>(h->seed >> 32);
    ulonglong2 *rows = h->slots<ulonglong2>();
    const int step_rows = 4 * (64 / lpr);
    for (int64_t p0 = 0; p0 < total; p0 += Pn) {
        const int Pc = static_cast<int>(std::min<int64_t>(Pn, total - p0)), Wc = 2 * Pc;
        const unsigned first_pair = static_cast<unsigned>(p0);
        if (sweep && pl.n_levels > 0) {
            const long long n0 = pl.level_rows[0];
            simu_init_kernel<<<static_cast<unsigned>((n0 * Pc + 255) / 256), 256, 0, h->stream>>>(h->d_state0, n0, rows, Pn, Pc);
            GENPHI_HIP_TRY(hipGetLastError());
            for (int k = 1; k < pl.n_levels; ++k) {
                const long long b = pl.level_begin[k];
                const int n_rows = static_cast<int>(pl.level_rows[k]);
                const unsigned grid = static_cast<unsigned>((n_rows + step_rows - 1) / step_rows);
                GENPHI_LPR_SWITCH(lpr, (simu_step_kernel<LPR><<<grid, 256, 0, h->stream>>>(h->d_fa + b, h->d_mo + b, h->d_ids + b, n_rows, b, rows, Pn, Pc,
                                                                                        first_pair, k0, k1)));
                GENPHI_HIP_TRY(hipGetLastError());
            }
        }
        if (results) {
            simu_states_kernel<<<static_cast<unsigned>((pl.n_pro + 3) / 4), 256, 0, h->stream>>>(rows, h->d_pro_row, pl.n_pro, Pn, Pc, first_pair, h->S, h->d_counts);
            GENPHI_HIP_TRY(hipGetLastError());
            if (!h->no_sample) {
                const long long threads = static_cast<long long>(pl.n_pro) * Wc;
                simu_sample_kernel<<<static_cast<unsigned>((threads + 255) / 256), 256, 0, h->stream>>>(reinterpret_cast<const u64 *>(rows), h->d_pro_row, pl.n_pro, Pn, Wc,
                                                                                                      2 * p0, h->S, h->d_sample);
                GENPHI_HIP_TRY(hipGetLastError());
            }
        }
        if (match) {
            const int wpr = lanes_per_row(Wc);
            const int rows_per_block = (256 / wpr) * SIMU_MATCH_ROWS;
            const dim3 grid(static_cast<unsigned>((pl.n_pro + rows_per_block - 1) / rows_per_block), static_cast<unsigned>((Wc + wpr - 1) / wpr));
            GENPHI_LPR_SWITCH(wpr, (simu_match_kernel<LPR><<<grid, 256, 0, h->stream>>>(reinterpret_cast<const u64 *>(rows), h->d_pro_row, h->d_state_pro, pl.n_pro, Pn,
                                                                                     Wc, 2 * p0, h->S, h->d_match)));
            GENPHI_HIP_TRY(hipGetLastError());
        }
    }
    return GENPHI_OK;
}

int compute_impl(genphi_simu *h, int32_t device)
{
    if (int rc = h->select(device)) return rc;
    if (int rc = prepare(h, h->device)) return rc;
    const genphi::SimuPlan &pl = h->plan;
    SweepRun run;
    if (int rc = run.begin(*h, 0.0)) return rc;
    GENPHI_HIP_TRY(hipMemsetAsync(h->d_counts, 0, h->d_counts.bytes(), h->stream));
    if (int rc = run_panels(h, true, true, false)) return rc;
    // per non-initial live row: two parent rows read and one written, 32 bytes per pair, over the panels
    const int64_t stepped = pl.n_live - (pl.n_levels ? pl.level_rows[0] : 0);
    run.bytes = 3.0 * 32.0 * static_cast<double>(stepped) * static_cast<double>(h->panels.total);
    run.launches = h->panels.n_panels * (pl.n_levels + 1 + (h->no_sample ? 0 : 1));
    return run.end(*h);
}

}  // namespace

extern "C" {

int genphi_simu_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro, const int64_t *pro_ids,
                       int64_t n_anc, const int64_t *anc_ids, const int32_t *anc_states, int64_t simul_no, uint64_t seed, int32_t flags,
                       genphi_simu **out)
{
    if (out) *out = nullptr;
    if (out && (flags & ~GENPHI_SIMU_FLAG_NO_SAMPLE)) return genphi_set_error(GENPHI_ERR_ARG, "genphi_simu_create: unknown flag");
    if (int rc = check_create_args("genphi_simu_create", n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids, out, INT32_MAX)) return rc;
    if (n_pro == 0) return genphi_set_error(GENPHI_ERR_ARG, "gen.simu: no probands");
    if (n_anc == 0) return genphi_set_error(GENPHI_ERR_ARG, "gen.simu: no ancestors");
    if (!anc_states) return genphi_set_error(GENPHI_ERR_ARG, "genphi_simu_create: anc_states is NULL");
    if (simul_no < 1 || simul_no > GENPHI_SIMU_MAX_SIMULATIONS)
        return genphi_set_error(GENPHI_ERR_ARG, "gen.simu: simulNo = " + std::to_string(simul_no) + " is outside 1 .. 2^24");
    return create_entry(out, "gen.simu", [&](genphi_simu *h) {
        h->S = simul_no;
        h->seed = seed;
        h->no_sample = (flags & GENPHI_SIMU_FLAG_NO_SAMPLE) != 0;
        h->panel_env = hook_count("GENPHI_SIMU_PANEL");
        std::string err;
        if (const int rc = genphi::plan_simu(h->plan, n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids, anc_states, err))
            return genphi_set_error(rc, err);
        return GENPHI_OK;
    });
}

int genphi_simu_levels(const genphi_simu *h, int64_t *n_live, int32_t *levels, int64_t *rows_per_level)
{
    return drop_levels(h, "genphi_simu_levels", n_live, levels, rows_per_level);
}

int genphi_simu_rows(const genphi_simu *h, int64_t *row_ids, int32_t *father_rows, int32_t *mother_rows, int64_t *pro_positions)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_simu_rows: NULL handle");
    const genphi::SimuPlan &pl = h->plan;
    if (row_ids) std::copy(pl.row_id.begin(), pl.row_id.end(), row_ids);
    if (father_rows) std::copy(pl.fa_row.begin(), pl.fa_row.end(), father_rows);
    if (mother_rows) std::copy(pl.mo_row.begin(), pl.mo_row.end(), mother_rows);
    if (pro_positions) std::copy(pl.pro_pos.begin(), pl.pro_pos.end(), pro_positions);
    return GENPHI_OK;
}

int genphi_simu_compute(genphi_simu *h, int32_t device) { return compute_entry(h, device, "genphi_simu_compute", "gen.simu", compute_impl); }

int genphi_simu_sample_to_host(genphi_simu *h, int8_t *out)
{
    if (h && h->computed && h->no_sample)    // (nothing computed comes first)
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_simu_sample_to_host: the handle was created with GENPHI_SIMU_FLAG_NO_SAMPLE");
    return result_to_host(h, out, &genphi_simu::d_sample, "genphi_simu_sample_to_host", "gen.simu");
}

int genphi_simu_state_counts(genphi_simu *h, int64_t *out)
{
    return result_to_host(h, out, &genphi_simu::d_counts, "genphi_simu_state_counts", "gen.simu");
}

int genphi_simu_match_counts(genphi_simu *h, const int32_t *state_pro, int32_t *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_simu_match_counts: nothing computed");
    if (!state_pro || !out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_simu_match_counts: NULL argument");
    for (size_t i = 0; i < h->d_state_pro.count(); ++i)
        if (state_pro[i] < 0 || state_pro[i] > 2)
            return genphi_set_error(GENPHI_ERR_ARG, "gen.simuProb: state " + std::to_string(state_pro[i]) + " of proband " + std::to_string(i) + " is outside 0..2");
    int rc = GENPHI_OK;
    const int drc = h->on_device("gen.simu match counts", [&] {
        hipError_t e = hipMemcpyAsync(h->d_state_pro, state_pro, h->d_state_pro.bytes(), hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) return e;
        e = hipMemsetAsync(h->d_match, 0, h->d_match.bytes(), h->stream);
        if (e != hipSuccess) return e;
        rc = run_panels(h, h->panels.n_panels > 1, false, true);            // one panel: its rows are resident
        if (rc) return hipSuccess;
        e = hipMemcpyAsync(out, h->d_match, h->d_match.bytes(), hipMemcpyDeviceToHost, h->stream);
        return e == hipSuccess ? hipStreamSynchronize(h->stream) : e;
    });
    return drc ? drc : rc;
}

int genphi_simu_stats(const genphi_simu *h, double *sweep_ms, double *algorithmic_bytes, int32_t *levels, int32_t *panel_cols, int64_t *panels,
                      int32_t *lanes_per_row, int64_t *n_live)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_simu_stats: NULL handle");
    h->stats(sweep_ms, algorithmic_bytes, nullptr);
    put(levels, h->plan.n_levels);
    put(panel_cols, 128 * h->panels.pairs);
    put(panels, h->panels.n_panels);
    put(lanes_per_row, h->panels.lanes_per_row);
    put(n_live, h->plan.n_live);
    return GENPHI_OK;
}

void genphi_simu_destroy(genphi_simu *h) { destroy_entry(h); }

}  // extern "C"
