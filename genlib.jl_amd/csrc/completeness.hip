// completeness.hip -- gen.completeness: ascents by generation (include/genphi.h, genphi_comp_*).
//
// Reference: completeness(pedigree, pro; genNo, type), src/describe.jl:73-125, walks every ascending path of every proband
// (_completeness!) and counts, per generation g, the known ancestors with multiplicity; entry = count / 2^g * 100.  The walk
// doubles per generation (genea140: 575,558 path steps for 140 probands).
//
// Here: the fifth recursion on the host schedule of ancestor_sweep.h, with GENERATIONS as the columns instead of ancestors:
//     P[x][0] = 1,    P[x][g] = P[father(x)][g - 1] + P[mother(x)][g - 1]      (a missing parent contributes nothing)
// P[x][g] = the number of ascending paths of exactly g meioses that start at x.  SweepOptions::every_member: every member of every
// cut has a row (no row is "none": column 0 is 1 for everybody), there is no ancestor list and no one-hot.
//
// Rows are Int64 counts, G = 1 + the longest ascent of a listed proband entries each (G <= 63, so a row is at most 504 bytes and
// there are no column panels), at a pitch of G rounded up to 8 entries (whole 64-byte lines).  P[x][g] <= 2^g <= 2^62: nothing
// overflows.  One item = one row, LPR lanes per row (the power of two >= G), one column per lane: lane g reads column g - 1 of
// both source rows -- the lanes of a row read 8-byte neighbours -- and writes column g; column 0 is the constant 1.  The step is a
// shift, so a proband that was dragged into the last cut (its row is final and waits in its slot) is a copy item
// (SweepOptions::mark_copies: source B = -2) that is written without the shift.
//
// The last list writes one result row per listed occurrence of every proband: the count, and the finished percentage by the
// reference's own two Float64 operations in its order, (double)count / 2^g * 100.0 (-ffp-contract=off): bit-identical to the
// reference.  Entries of generations beyond a proband's own depth are 0.0, generation 0 is 100.0.
//   totals   per generation, the counts summed over the result rows (each listed occurrence counts), on the device: the column sums
//            of the resident counts, or -- GENPHI_COMP_FLAG_TOTALS_ONLY, no (n_pro, G) buffer exists -- the last list reduced as
//            genphi_occ_totals reduces it (partial sums of COMP_TOTAL_ROWS rows in registers, then 64-bit integer atomics: the
//            same bits on every run).  A total is at most n_pro 2^(G - 1): it cannot overflow while (G - 1) + ceil(log2(n_pro)) <= 62.
#include <hip/hip_runtime.h>

#include "sweep_device.h"

namespace {

static_assert(sizeof(genphi::SweepItem) == sizeof(int4), "items are uploaded as they are and read as int4");

// column g of the row of one item: 1 in column 0, else the sum of column g - 1 of the sources; a copy item: column g of source A
__device__ __forceinline__ long long comp_entry(const int4 it, const long long *__restrict__ slots, int pitch, int g)
{
    const bool copy = it.z == -2;
    if (g == 0 && !copy) return 1;
    const int s = copy ? g : g - 1;
    long long v = 0;
    if (it.y >= 0) v = slots[static_cast<long long>(it.y) * pitch + s];
    if (it.z >= 0) v += slots[static_cast<long long>(it.z) * pitch + s];
    return v;
}

// One item = one row, LPR lanes per row (a power of two >= G), lane g owns column g; a wave holds 64 / LPR rows.
// TO_RESULT: the row goes to result row it.x of the counts and of the percentages (G entries per row, packed).
template <int LPR, bool TO_RESULT>
__global__ void __launch_bounds__(256)
comp_step_kernel(const int4 *__restrict__ items, int n_items, long long *__restrict__ slots, int pitch, int G,
                 long long *__restrict__ counts, double *__restrict__ pct)
{
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long item = (static_cast<long long>(blockIdx.x) * 4 + wave) * RPW + lane / LPR;
    if (item >= n_items) return;
    const int g = lane % LPR;
    if (g >= G) return;
    const int4 it = items[item];
    const long long v = comp_entry(it, slots, pitch, g);
    if (TO_RESULT) {
        const long long o = static_cast<long long>(it.x) * G + g;
        counts[o] = v;
        pct[o] = static_cast<double>(v) / static_cast<double>(1ull << g) * 100.0;     // the reference's operations, in its order
    } else {
        slots[static_cast<long long>(it.x) * pitch + g] = v;
    }
}

// Totals only: the items of the last list, COMP_TOTAL_ROWS consecutive items per row group (LPR lanes), summed in a register per
// column, then one 64-bit atomic add per column and row group.
constexpr int COMP_TOTAL_ROWS = 64;

template <int LPR>
__global__ void __launch_bounds__(256)
comp_total_kernel(const int4 *__restrict__ items, int n_items, const long long *__restrict__ slots, int pitch, int G,
                  unsigned long long *__restrict__ totals)
{
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long first = ((static_cast<long long>(blockIdx.x) * 4 + wave) * RPW + lane / LPR) * COMP_TOTAL_ROWS;
    if (first >= n_items) return;
    const int last = static_cast<int>(min(first + COMP_TOTAL_ROWS, static_cast<long long>(n_items)));
    const int g = lane % LPR;
    if (g >= G) return;
    unsigned long long acc = 0;
    for (int i = static_cast<int>(first); i < last; ++i) acc += static_cast<unsigned long long>(comp_entry(items[i], slots, pitch, g));
    if (acc) atomicAdd(&totals[g], acc);
}

// Totals of a resident result: column sums of the n_rows x G counts (lane g owns column g, the 4 waves of a block share 1,024 rows).
__global__ void __launch_bounds__(256)
comp_colsum_kernel(const long long *__restrict__ counts, long long n_rows, int G, unsigned long long *__restrict__ totals)
{
    const int g = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (g >= G) return;
    const long long r0 = static_cast<long long>(blockIdx.x) * 1024, r1 = min(r0 + 1024, n_rows);
    unsigned long long s = 0;
    for (long long r = r0 + wave; r < r1; r += 4) s += static_cast<unsigned long long>(counts[r * G + g]);
    if (s) atomicAdd(&totals[g], s);
}

// Int64 rows at a pitch of 8 entries (rows start on 64 bytes); one panel of every generation: nothing is sized
constexpr genphi::PanelRule kCompRows = {8, 1, 8, 1, 1, 0, 1};

}  // namespace

struct genphi_comp : SweepDevice {
    int64_t n_pro = 0;
    int32_t G = 0, pitch = 0;                // generations (result columns), entries per slot row
    bool totals_only = false;
    genphi::SweepSchedule sched;             // host schedule (ancestor_sweep.h)
    DevBuf<long long> d_counts;              // n_pro x G (not on a totals-only handle)
    DevBuf<double> d_result;                 // n_pro x G percentages (not on a totals-only handle)
    DevBuf<unsigned long long> d_totals;     // G totals (a totals-only handle: written by the sweep; else on request)
    DevBuf<int4> d_items;
    bool totals_ready = false;
    genphi_comp() { own(d_counts, d_result, d_totals, d_items); }
    size_t result_entries() const { return static_cast<size_t>(n_pro) * static_cast<size_t>(G); }
    bool empty() const { return n_pro == 0 || G == 0; }
    // a total is at most n_pro 2^(G - 1)
    bool totals_fit() const
    {
        int bits = 0;
        while ((int64_t(1) << bits) < n_pro) ++bits;
        return (G - 1) + bits <= 62;
    }
};

namespace {

int compute_impl(genphi_comp *h, int32_t device)
{
    if (int rc = h->select(device)) return rc;
    h->totals_ready = false;
    const int G = h->G, pitch = h->pitch;
    const size_t n_res = h->totals_only ? 0 : h->result_entries();
    genphi::PanelLayout L;
    L.slots = std::max<int64_t>(h->sched.peak_slots, 1);
    L.C = G; L.Cp = pitch; L.n_panels = 1; L.per_launch = 1;
    L.stride = static_cast<long long>(L.slots) * pitch;
    L.slot_bytes = static_cast<size_t>(L.stride) * sizeof(long long);
    if (!h->d_slots.get()) {
        double usable = 0.0;
        if (int rc = h->usable_bytes(usable, 0)) return rc;
        const double need = static_cast<double>(L.slot_bytes) + 16.0 * static_cast<double>(n_res) + 16.0 * static_cast<double>(h->sched.items.size()) + (64 << 20);
        if (need > usable)
            return genphi_set_error(GENPHI_ERR_ALLOC, "gen.completeness: " + std::to_string(static_cast<size_t>(need) >> 20) +
                                                          " MiB of slot rows and result do not fit on device " + std::to_string(device));
        GENPHI_HIP_TRY(h->d_slots.reserve(L.slot_bytes));
    }
    GENPHI_HIP_TRY(h->d_totals.reserve(static_cast<size_t>(G)));
    if (n_res) {
        GENPHI_HIP_TRY(h->d_counts.reserve(n_res));
        GENPHI_HIP_TRY(h->d_result.reserve(n_res));
    }
    if (int rc = h->upload(h->d_items, h->sched.items)) return rc;
    const double row_bytes = 8.0 * G;
    SweepRun run;
    if (int rc = run.begin(*h, h->totals_only ? row_bytes : 2.0 * row_bytes * static_cast<double>(h->n_pro))) return rc;
    // (every listed proband is in the last list: each result row is written whole, nothing is pre-filled)
    if (h->totals_only) GENPHI_HIP_TRY(hipMemsetAsync(h->d_totals, 0, h->d_totals.bytes(), h->stream));
    const int lpr = lanes_per_row(G);
    long long *slots = h->slots<long long>();
    auto launch = [&](const ListLaunch &l) {
        if (!l.to_result) {
            GENPHI_LPR_SWITCH(lpr, (comp_step_kernel<LPR, false><<<l.grid.x, 256, 0, h->stream>>>(l.items, l.n_items, slots, pitch, G, nullptr, nullptr)));
        } else if (h->totals_only) {
            GENPHI_LPR_SWITCH(lpr, (comp_total_kernel<LPR><<<l.grid.x, 256, 0, h->stream>>>(l.items, l.n_items, slots, pitch, G, h->d_totals)));
        } else {
            GENPHI_LPR_SWITCH(lpr, (comp_step_kernel<LPR, true><<<l.grid.x, 256, 0, h->stream>>>(l.items, l.n_items, slots, pitch, G, h->d_counts, h->d_result)));
        }
    };
    if (int rc = sweep_lists(run, h->sched, h->d_items, kCompRows, L, G, 4 * (64 / lpr), h->totals_only ? COMP_TOTAL_ROWS : 1, launch)) return rc;
    if (int rc = run.end(*h)) return rc;
    h->totals_ready = h->totals_only;
    return GENPHI_OK;
}

}  // namespace

extern "C" {

int genphi_comp_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                       const int64_t *pro_ids, int32_t flags, genphi_comp **out)
{
    if (out) *out = nullptr;
    if (out && (flags & ~GENPHI_COMP_FLAG_TOTALS_ONLY)) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_create: unknown flag");
    if (int rc = check_create_args("genphi_comp_create", n_ind, ind, father, mother, n_pro, pro_ids, 0, nullptr, out, 0)) return rc;
    return create_entry(out, "gen.completeness", [&](genphi_comp *h) {
        genphi::SweepOptions opt;
        opt.emit = genphi::Emit::EveryProband;
        opt.mark_copies = true;
        opt.every_member = true;
        std::string err;
        if (const int rc = genphi::plan_sweep(h->sched, n_ind, ind, father, mother, n_pro, pro_ids, 0, nullptr, opt, err)) return genphi_set_error(rc, err);
        h->n_pro = h->sched.n_pro;
        h->G = h->sched.n_generations;
        h->totals_only = (flags & GENPHI_COMP_FLAG_TOTALS_ONLY) != 0;
        if (h->G - 1 > GENPHI_COMP_MAX_GENERATIONS)
            return genphi_set_error(GENPHI_ERR_ARG, "gen.completeness: " + std::to_string(h->G - 1) + " generations above the probands; Int64 counts (and the reference's 2^g) hold at most " +
                                                        std::to_string(GENPHI_COMP_MAX_GENERATIONS));
        if (h->totals_only && !h->totals_fit())
            return genphi_set_error(GENPHI_ERR_ARG, "gen.completeness: the totals of " + std::to_string(h->n_pro) + " probands over " + std::to_string(h->G) +
                                                        " generations can exceed Int64; sum the per-proband result instead");
        h->pitch = static_cast<int32_t>(kCompRows.pitch(h->G));
        return GENPHI_OK;
    });
}

int genphi_comp_compute(genphi_comp *h, int32_t device) { return compute_entry(h, device, "genphi_comp_compute", "gen.completeness", compute_impl); }

int genphi_comp_generations(const genphi_comp *h, int32_t *generations)
{
    if (!h || !generations) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_generations: NULL argument");
    *generations = h->G;
    return GENPHI_OK;
}

int genphi_comp_result_device(const genphi_comp *h, const double **d_ptr, int64_t *ld)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_result_device: nothing computed");
    if (h->totals_only) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_result_device: a totals-only handle has no n_pro x G result");
    put(d_ptr, h->d_result.get());
    put(ld, h->G);
    return GENPHI_OK;
}

int genphi_comp_result_to_host(genphi_comp *h, double *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_result_to_host: nothing computed");
    if (h->totals_only) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_result_to_host: a totals-only handle has no n_pro x G result");
    if (h->empty()) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_result_to_host: out is NULL");
    return h->copy_out(out, h->d_result, h->d_result.bytes(), "gen.completeness");
}

int genphi_comp_counts_to_host(genphi_comp *h, int64_t *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_counts_to_host: nothing computed");
    if (h->totals_only) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_counts_to_host: a totals-only handle has no n_pro x G result");
    if (h->empty()) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_counts_to_host: out is NULL");
    return h->copy_out(out, h->d_counts, h->d_counts.bytes(), "gen.completeness");
}

int genphi_comp_totals(genphi_comp *h, int64_t *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_totals: nothing computed");
    if (h->empty()) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_totals: out is NULL");
    if (!h->totals_fit()) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_totals: the totals can exceed Int64; sum the per-proband result instead");
    const size_t bytes = static_cast<size_t>(h->G) * sizeof(int64_t);
    if (!h->totals_ready) {
        // a handle with a full result: the column sums of the resident counts
        const int rc = h->on_device("gen.completeness totals", [&] {
            const hipError_t e = hipMemsetAsync(h->d_totals, 0, bytes, h->stream);
            if (e != hipSuccess) return e;
            comp_colsum_kernel<<<static_cast<unsigned>((h->n_pro + 1023) / 1024), 256, 0, h->stream>>>(h->d_counts, h->n_pro, h->G, h->d_totals);
            return hipGetLastError();
        });
        if (rc) return rc;
        h->totals_ready = true;
    }
    return h->copy_out(out, h->d_totals, bytes, "gen.completeness");
}

int genphi_comp_stats(const genphi_comp *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *row_entries,
                      int64_t *launches)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_stats: NULL handle");
    h->stats(sweep_ms, algorithmic_bytes, launches);
    put(peak_slots, h->sched.peak_slots);
    put(row_entries, h->pitch);
    return GENPHI_OK;
}

void genphi_comp_destroy(genphi_comp *h) { destroy_entry(h); }

}  // extern "C"
