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

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/genphi.h"
#include "ancestor_sweep.h"
#include "devcache.h"
#include "planner.h"

int genphi_set_error(int code, const std::string &msg);      // genphi_hip.hip

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

#define COMP_LPR_SWITCH(lpr, CALL)                     \
    switch (lpr) {                                     \
    case 1: { constexpr int LPR = 1; CALL; } break;    \
    case 2: { constexpr int LPR = 2; CALL; } break;    \
    case 4: { constexpr int LPR = 4; CALL; } break;    \
    case 8: { constexpr int LPR = 8; CALL; } break;    \
    case 16: { constexpr int LPR = 16; CALL; } break;  \
    case 32: { constexpr int LPR = 32; CALL; } break;  \
    default: { constexpr int LPR = 64; CALL; } break;  \
    }

constexpr int64_t kPitchEntries = 8;     // rows start on 64 bytes

}  // namespace

struct genphi_comp {
    int64_t n_pro = 0;
    int32_t G = 0, pitch = 0;                // generations (result columns), entries per slot row
    bool totals_only = false;
    genphi::SweepSchedule sched;             // host schedule (ancestor_sweep.h)
    // device
    int device = -1;
    hipStream_t stream = nullptr;
    long long *d_counts = nullptr;           // n_pro x G (not on a totals-only handle)
    double *d_result = nullptr;              // n_pro x G percentages (not on a totals-only handle)
    unsigned long long *d_totals = nullptr;  // G totals (a totals-only handle: written by the sweep; else on request)
    int4 *d_items = nullptr;
    long long *d_slots = nullptr;
    bool computed = false, totals_ready = false;
    double sweep_ms = 0.0, alg_bytes = 0.0;
    int64_t n_launches = 0;
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

void release_device(genphi_comp *h)
{
    if (h->device < 0) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    (void)genphi::cached_free(h->d_counts);
    (void)genphi::cached_free(h->d_result);
    (void)genphi::cached_free(h->d_totals);
    (void)genphi::cached_free(h->d_items);
    (void)genphi::cached_free(h->d_slots);
    h->d_counts = nullptr; h->d_result = nullptr; h->d_totals = nullptr; h->d_items = nullptr; h->d_slots = nullptr;
    if (h->stream) genphi::cached_stream_release(h->stream, h->device);
    h->stream = nullptr;
    (void)hipSetDevice(cur);
    h->device = -1;
    h->computed = false; h->totals_ready = false;
}

#define COMP_TRY(expr)                                                                                          \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

int lanes_per_row(int cols)
{
    int lpr = 1;
    while (lpr < cols && lpr < 64) lpr *= 2;
    return lpr;
}

int compute_impl(genphi_comp *h, int32_t device)
{
    if (device < 0) COMP_TRY(hipGetDevice(&device));
    if (h->device >= 0 && h->device != device) release_device(h);
    COMP_TRY(hipSetDevice(device));
    h->device = device;
    h->computed = false; h->totals_ready = false;
    if (!h->stream) COMP_TRY(genphi::cached_stream(&h->stream));
    const int G = h->G, pitch = h->pitch;
    const size_t n_res = h->totals_only ? 0 : h->result_entries();
    const size_t slot_bytes = static_cast<size_t>(std::max<int64_t>(h->sched.peak_slots, 1)) * static_cast<size_t>(pitch) * sizeof(long long);
    const size_t item_bytes = h->sched.items.size() * sizeof(int4);
    if (!h->d_slots) {
        size_t free_b = 0, total_b = 0;
        COMP_TRY(hipMemGetInfo(&free_b, &total_b));
        const double need = static_cast<double>(slot_bytes) + 16.0 * static_cast<double>(n_res) + static_cast<double>(item_bytes) + (64 << 20);
        if (need > 0.9 * static_cast<double>(free_b))
            return genphi_set_error(GENPHI_ERR_ALLOC, "gen.completeness: " + std::to_string(static_cast<size_t>(need) >> 20) +
                                                          " MiB of slot rows and result do not fit on device " + std::to_string(device));
        COMP_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_slots), slot_bytes));
    }
    if (!h->d_totals) COMP_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_totals), static_cast<size_t>(G) * sizeof(unsigned long long)));
    if (n_res && !h->d_counts) COMP_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_counts), n_res * sizeof(long long)));
    if (n_res && !h->d_result) COMP_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_result), n_res * sizeof(double)));
    if (!h->d_items) {
        COMP_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_items), item_bytes));
        COMP_TRY(hipMemcpyAsync(h->d_items, h->sched.items.data(), item_bytes, hipMemcpyHostToDevice, h->stream));
    }
    hipEvent_t e0, e1;
    COMP_TRY(hipEventCreate(&e0));
    COMP_TRY(hipEventCreate(&e1));
    COMP_TRY(hipEventRecord(e0, h->stream));
    // (every listed proband is in the last list: each result row is written whole, nothing is pre-filled)
    if (h->totals_only) COMP_TRY(hipMemsetAsync(h->d_totals, 0, static_cast<size_t>(G) * sizeof(unsigned long long), h->stream));
    const int lpr = lanes_per_row(G);
    const int rows_per_block = 4 * (64 / lpr);
    const int n_lists = static_cast<int>(h->sched.list_to_result.size());
    const double row_bytes = 8.0 * G;
    double bytes = h->totals_only ? row_bytes : 2.0 * row_bytes * static_cast<double>(h->n_pro);
    int64_t launches = 0;
    for (int k = 0; k < n_lists; ++k) {
        const int64_t b = h->sched.list_begin[k], n_items = h->sched.list_begin[k + 1] - 1 - b;
        if (n_items <= 0) continue;
        const bool to_res = h->sched.list_to_result[k];
        bytes += row_bytes * (h->sched.list_srcs[k] + (to_res ? 0.0 : static_cast<double>(n_items)));
        const int64_t units = to_res && h->totals_only ? (n_items + COMP_TOTAL_ROWS - 1) / COMP_TOTAL_ROWS : n_items;
        const unsigned grid = static_cast<unsigned>((units + rows_per_block - 1) / rows_per_block);
        const int4 *items = h->d_items + b;
        const int n = static_cast<int>(n_items);
        if (!to_res) {
            COMP_LPR_SWITCH(lpr, (comp_step_kernel<LPR, false><<<grid, 256, 0, h->stream>>>(items, n, h->d_slots, pitch, G, nullptr, nullptr)));
        } else if (h->totals_only) {
            COMP_LPR_SWITCH(lpr, (comp_total_kernel<LPR><<<grid, 256, 0, h->stream>>>(items, n, h->d_slots, pitch, G, h->d_totals)));
        } else {
            COMP_LPR_SWITCH(lpr, (comp_step_kernel<LPR, true><<<grid, 256, 0, h->stream>>>(items, n, h->d_slots, pitch, G, h->d_counts, h->d_result)));
        }
        COMP_TRY(hipGetLastError());
        ++launches;
    }
    COMP_TRY(hipEventRecord(e1, h->stream));
    COMP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    COMP_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    h->sweep_ms = ms;
    h->alg_bytes = bytes;
    h->n_launches = launches;
    h->computed = true;
    h->totals_ready = h->totals_only;
    return GENPHI_OK;
}

// bytes from the device (src) to the host
int copy_out(genphi_comp *h, void *out, const void *src, size_t bytes)
{
    int cur = 0;
    COMP_TRY(hipGetDevice(&cur));
    COMP_TRY(hipSetDevice(h->device));
    const hipError_t e = hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, h->stream);
    const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(h->stream) : e;
    (void)hipSetDevice(cur);
    if (e2 != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string("gen.completeness result copy: ") + hipGetErrorString(e2));
    return GENPHI_OK;
}

}  // namespace

extern "C" {

int genphi_comp_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                       const int64_t *pro_ids, int32_t flags, genphi_comp **out)
{
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_create: out is NULL");
    *out = nullptr;
    if (flags & ~GENPHI_COMP_FLAG_TOTALS_ONLY) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_create: unknown flag");
    if (n_ind < 0 || n_pro < 0 || (n_ind && (!ind || !father || !mother)) || (n_pro && !pro_ids))
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_create: bad sizes or NULL arrays");
    if (n_ind >= INT32_MAX || n_pro >= INT32_MAX)
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_create: more than 2^31 - 2 individuals or probands");
    genphi_comp *h = new (std::nothrow) genphi_comp();
    if (!h) return genphi_set_error(GENPHI_ERR_ALLOC, "out of memory");
    int rc;
    try {
        genphi::SweepOptions opt;
        opt.emit = genphi::Emit::EveryProband;
        opt.mark_copies = true;
        opt.every_member = true;
        std::string err;
        rc = genphi::plan_sweep(h->sched, n_ind, ind, father, mother, n_pro, pro_ids, 0, nullptr, opt, err);
        h->n_pro = h->sched.n_pro;
        h->G = h->sched.n_generations;
        h->totals_only = (flags & GENPHI_COMP_FLAG_TOTALS_ONLY) != 0;
        if (rc) rc = genphi_set_error(rc, err);
        else if (h->G - 1 > GENPHI_COMP_MAX_GENERATIONS)
            rc = genphi_set_error(GENPHI_ERR_ARG, "gen.completeness: " + std::to_string(h->G - 1) + " generations above the probands; Int64 counts (and the reference's 2^g) hold at most " +
                                                      std::to_string(GENPHI_COMP_MAX_GENERATIONS));
        else if (h->totals_only && !h->totals_fit())
            rc = genphi_set_error(GENPHI_ERR_ARG, "gen.completeness: the totals of " + std::to_string(h->n_pro) + " probands over " + std::to_string(h->G) +
                                                      " generations can exceed Int64; sum the per-proband result instead");
    } catch (const std::bad_alloc &) { rc = genphi_set_error(GENPHI_ERR_ALLOC, "out of memory while planning gen.completeness"); }
    if (rc) { delete h; return rc; }
    h->pitch = static_cast<int32_t>((h->G + kPitchEntries - 1) / kPitchEntries * kPitchEntries);
    *out = h;
    return GENPHI_OK;
}

int genphi_comp_compute(genphi_comp *h, int32_t device)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_compute: NULL handle");
    if (h->empty()) { h->computed = true; h->sweep_ms = 0.0; h->alg_bytes = 0.0; h->n_launches = 0; return GENPHI_OK; }
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, "gen.completeness: no usable GPU");
    int rc;
    try {
        rc = compute_impl(h, device);
    } catch (const std::bad_alloc &) { rc = genphi_set_error(GENPHI_ERR_ALLOC, "out of host memory in gen.completeness"); }
    (void)hipSetDevice(cur);
    return rc;
}

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
    if (d_ptr) *d_ptr = h->d_result;
    if (ld) *ld = h->G;
    return GENPHI_OK;
}

int genphi_comp_result_to_host(genphi_comp *h, double *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_result_to_host: nothing computed");
    if (h->totals_only) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_result_to_host: a totals-only handle has no n_pro x G result");
    if (h->empty()) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_result_to_host: out is NULL");
    return copy_out(h, out, h->d_result, h->result_entries() * sizeof(double));
}

int genphi_comp_counts_to_host(genphi_comp *h, int64_t *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_counts_to_host: nothing computed");
    if (h->totals_only) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_counts_to_host: a totals-only handle has no n_pro x G result");
    if (h->empty()) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_counts_to_host: out is NULL");
    return copy_out(h, out, h->d_counts, h->result_entries() * sizeof(long long));
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
        int cur = 0;
        COMP_TRY(hipGetDevice(&cur));
        COMP_TRY(hipSetDevice(h->device));
        hipError_t e = hipMemsetAsync(h->d_totals, 0, bytes, h->stream);
        if (e == hipSuccess) {
            comp_colsum_kernel<<<static_cast<unsigned>((h->n_pro + 1023) / 1024), 256, 0, h->stream>>>(h->d_counts, h->n_pro, h->G, h->d_totals);
            e = hipGetLastError();
        }
        (void)hipSetDevice(cur);
        if (e != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string("gen.completeness totals: ") + hipGetErrorString(e));
        h->totals_ready = true;
    }
    return copy_out(h, out, h->d_totals, bytes);
}

int genphi_comp_stats(const genphi_comp *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *row_entries,
                      int64_t *launches)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_comp_stats: NULL handle");
    if (sweep_ms) *sweep_ms = h->sweep_ms;
    if (algorithmic_bytes) *algorithmic_bytes = h->alg_bytes;
    if (peak_slots) *peak_slots = h->sched.peak_slots;
    if (row_entries) *row_entries = h->pitch;
    if (launches) *launches = h->n_launches;
    return GENPHI_OK;
}

void genphi_comp_destroy(genphi_comp *h)
{
    if (!h) return;
    release_device(h);
    delete h;
}

}  // extern "C"
