// gc.hip -- gen.gc: the genetic contribution of ancestors to probands (include/genphi.h, genphi_gc_*).
//
// Reference: gc(pedigree; pro, ancestors), src/compute.jl:518-595 (GENLIB's Congen).  For every ancestor it walks every
// descending path to every leaf below it (_contribute!, :531-540) and adds 0.5^length to the leaf; a proband's Float32
// accumulator is read into its row and reset after each ancestor.  One step per path: 287,849 paths on genea140, about 2^29 per
// leaf on cfg4.
//
// Here: the same numbers from a linear recursion over the generation cuts of the planner (build_plan, indices_only):
//     row[x] = 0.5 * (row[father] + row[mother])  (a missing parent is the zero row),  then row[x][j] = 1 for every column j with
//     ancestors[j] == x
// Row x, column j = sum over the paths from ancestors[j] down to x of 0.5^length.  Every path into cut c has at most c steps, so
// the values of cut c are multiples of 2^-c in [0, 1]: the Float64 rows are exact for up to 52 steps, and the result is rounded
// to Float32 once (see the contract in include/genphi.h).
//
// Host schedule (genphi_gc_create, no GPU):
//   rows    only members that are a requested ancestor or descend from one are computed; every other row is zero ("none")
//   slots   each computed member owns one Float64 row of a slot buffer from the step that creates it until its last cut has been
//           read; members dragged from one cut to the next keep their slot (nothing is copied); a slot freed after step s is
//           handed out from step s+1 on, never inside the launch that still reads it
//   emit    the last step writes its rows straight into the Float32 result (n_pro x n_anc, row-major, ld = n_anc): only the first
//           occurrence of a leaf proband gets values; the result is cleared once before the sweep
// Column panels: the columns are independent; a sweep runs over panels of C ancestor columns (slot memory peak_slots x C x 8
// bytes per panel).  A launch can cover several panels through grid dimension y; by default panels are sized for the Infinity
// Cache and swept one after the other (kPanelSlotBytes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/genphi.h"
#include "devcache.h"
#include "planner.h"

int genphi_set_error(int code, const std::string &msg);      // genphi_hip.hip

namespace {

// One item = one row a launch computes: (destination slot or result row, source slot A, source slot B, first one-hot entry);
// -1 = the zero row.  The one-hot entries of item i are oh_cols[items[i].w .. items[i + 1].w) (global column indices,
// ascending); every list of items ends with a sentinel whose .w closes the last one.
//
// LPR lanes per row (a power of two): each lane moves 16 bytes (two Float64 columns) per access, U accesses of each source row
// in flight before any is used; a wave holds 64 / LPR rows (narrow panels: several rows per wave instead of idle lanes).
template <int LPR, bool TO_RESULT>
__global__ void __launch_bounds__(256)
gc_step_kernel(const int4 *__restrict__ items, const int *__restrict__ oh_cols, int n_items, double *__restrict__ slots,
               long long panel_stride, int Cp, int C, int n_anc, int panel0, float *__restrict__ out)
{
    constexpr int RPW = 64 / LPR;
    constexpr int U = 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long item = (static_cast<long long>(blockIdx.x) * 4 + wave) * RPW + lane / LPR;
    if (item >= n_items) return;
    const int l = lane % LPR;
    const int panel = panel0 + static_cast<int>(blockIdx.y);
    const int p0 = panel * C;
    const int ncols = min(C, n_anc - p0);
    const int lim = (ncols + 1) & ~1;                      // columns moved: the panel's, rounded up to a 16-byte pair
    const int4 it = items[item];
    const int oh_b = it.w, oh_e = items[item + 1].w;
    double *base = slots + static_cast<long long>(blockIdx.y) * panel_stride;
    const double2 *rA = it.y >= 0 ? reinterpret_cast<const double2 *>(base + static_cast<long long>(it.y) * Cp) : nullptr;
    const double2 *rB = it.z >= 0 ? reinterpret_cast<const double2 *>(base + static_cast<long long>(it.z) * Cp) : nullptr;
    double2 *dst = TO_RESULT ? nullptr : reinterpret_cast<double2 *>(base + static_cast<long long>(it.x) * Cp);
    float *orow = TO_RESULT ? out + static_cast<long long>(it.x) * n_anc + p0 : nullptr;
    for (int c0 = 2 * l; c0 < lim; c0 += 2 * LPR * U) {
        double2 a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * 2 * LPR;
            a[u] = make_double2(0.0, 0.0);
            b[u] = make_double2(0.0, 0.0);
            if (c < lim) {
                if (rA) a[u] = rA[c >> 1];
                if (rB) b[u] = rB[c >> 1];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * 2 * LPR;
            if (c >= lim) break;
            double2 v = make_double2(0.5 * (a[u].x + b[u].x), 0.5 * (a[u].y + b[u].y));
            for (int k = oh_b; k < oh_e; ++k) {
                const int j = oh_cols[k] - p0;
                if (j == c) v.x = 1.0;
                if (j == c + 1 && c + 1 < ncols) v.y = 1.0;
            }
            if (TO_RESULT) {
                // rows of the result are not 16-byte (or 8-byte) aligned when n_anc is odd: two 4-byte stores
                orow[c] = static_cast<float>(v.x);
                if (c + 1 < ncols) orow[c + 1] = static_cast<float>(v.y);
            } else {
                dst[c >> 1] = v;
            }
        }
    }
}

template <bool TO_RESULT>
void launch_step(int lpr, dim3 grid, hipStream_t st, const int4 *items, const int *oh, int n_items, double *slots, long long stride,
                 int Cp, int C, int n_anc, int panel0, float *out)
{
    switch (lpr) {
    case 1: gc_step_kernel<1, TO_RESULT><<<grid, 256, 0, st>>>(items, oh, n_items, slots, stride, Cp, C, n_anc, panel0, out); break;
    case 2: gc_step_kernel<2, TO_RESULT><<<grid, 256, 0, st>>>(items, oh, n_items, slots, stride, Cp, C, n_anc, panel0, out); break;
    case 4: gc_step_kernel<4, TO_RESULT><<<grid, 256, 0, st>>>(items, oh, n_items, slots, stride, Cp, C, n_anc, panel0, out); break;
    case 8: gc_step_kernel<8, TO_RESULT><<<grid, 256, 0, st>>>(items, oh, n_items, slots, stride, Cp, C, n_anc, panel0, out); break;
    case 16: gc_step_kernel<16, TO_RESULT><<<grid, 256, 0, st>>>(items, oh, n_items, slots, stride, Cp, C, n_anc, panel0, out); break;
    case 32: gc_step_kernel<32, TO_RESULT><<<grid, 256, 0, st>>>(items, oh, n_items, slots, stride, Cp, C, n_anc, panel0, out); break;
    default: gc_step_kernel<64, TO_RESULT><<<grid, 256, 0, st>>>(items, oh, n_items, slots, stride, Cp, C, n_anc, panel0, out); break;
    }
}

// Default panels: as wide as keeps the slot rows of one panel within about 150 MiB, so that a panel's live rows stay in the
// 256 MiB Infinity Cache between the step that writes them and the steps that read them; one panel per launch, panels one after
// the other.  Measured against one panel of every column: cfg3 x 6,633 founders 1.53 vs 1.96 ms, cfg4 x
// 50,366 founders 122 vs 140 ms.  Narrower than kPanelMinCols the rows get too short for the 16-byte row gather.
constexpr double kPanelSlotBytes = 150.0 * 1048576.0;
constexpr int64_t kPanelMinCols = 64;

}  // namespace

struct genphi_gc {
    int64_t n_pro = 0, n_anc = 0;
    // host schedule
    std::vector<int4> items;                 // every launch's items, each list closed by a sentinel
    std::vector<int32_t> oh_cols;
    std::vector<int64_t> list_begin;         // launch k: items [list_begin[k], list_begin[k + 1] - 1) (the last one a sentinel)
    std::vector<char> list_to_result;
    std::vector<double> list_srcs;           // source rows read, summed over the list's items (algorithmic bytes)
    int64_t peak_slots = 0;
    int32_t panel_env = 0, group_env = 0;    // GENPHI_GC_PANEL / GENPHI_GC_PANELS_PER_LAUNCH (0 = default rule)
    // device
    int device = -1;
    hipStream_t stream = nullptr;
    float *d_result = nullptr;
    int4 *d_items = nullptr;
    int *d_oh = nullptr;
    double *d_slots = nullptr;
    size_t slot_bytes = 0;
    bool computed = false;
    double sweep_ms = 0.0, alg_bytes = 0.0;
    int32_t panel_cols = 0;
};

namespace {

void release_device(genphi_gc *h)
{
    if (h->device < 0) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    (void)genphi::cached_free(h->d_result);
    (void)genphi::cached_free(h->d_items);
    (void)genphi::cached_free(h->d_oh);
    (void)genphi::cached_free(h->d_slots);
    h->d_result = nullptr; h->d_items = nullptr; h->d_oh = nullptr; h->d_slots = nullptr; h->slot_bytes = 0;
    if (h->stream) genphi::cached_stream_release(h->stream, h->device);
    h->stream = nullptr;
    (void)hipSetDevice(cur);
    h->device = -1;
    h->computed = false;
}

#define GC_TRY(expr)                                                                                            \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// ID -> rank (a direct table for dense non-negative IDs, else a hash map)
struct Ranks {
    std::vector<int32_t> table;
    std::unordered_map<int64_t, int32_t> map;
    bool direct = false;
    void init(int64_t n, const int64_t *ind)
    {
        int64_t lo = INT64_MAX, hi = INT64_MIN;
        for (int64_t i = 0; i < n; ++i) { lo = std::min(lo, ind[i]); hi = std::max(hi, ind[i]); }
        direct = n > 0 && lo >= 0 && hi < 3 * n + 1024;
        if (direct) {
            table.assign(static_cast<size_t>(hi) + 1, -1);
            for (int64_t i = 0; i < n; ++i) table[ind[i]] = static_cast<int32_t>(i);
        } else {
            map.reserve(static_cast<size_t>(n) * 2);
            for (int64_t i = 0; i < n; ++i) map.emplace(ind[i], static_cast<int32_t>(i));
        }
    }
    int32_t find(int64_t id) const
    {
        if (direct) return (id < 0 || id >= static_cast<int64_t>(table.size())) ? -1 : table[id];
        auto it = map.find(id);
        return it == map.end() ? -1 : it->second;
    }
};

int plan_gc(genphi_gc *h, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
            const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids)
{
    genphi::PlanOptions opt;
    opt.indices_only = true;
    genphi::Plan plan;
    std::string err;
    // (validates the pedigree -- order, duplicates -- and the proband IDs; the planner keeps first occurrences)
    int rc = genphi::build_plan(n_ind, ind, father, mother, n_pro, pro_ids, opt, plan, err);
    if (rc) return genphi_set_error(rc, err);
    Ranks ranks;
    ranks.init(n_ind, ind);
    std::vector<int32_t> anc_rank(n_anc);
    for (int64_t j = 0; j < n_anc; ++j) {
        anc_rank[j] = ranks.find(anc_ids[j]);
        if (anc_rank[j] < 0) return genphi_set_error(GENPHI_ERR_UNKNOWN_ID, "KeyError: ancestor " + std::to_string(anc_ids[j]) + " not found");
    }
    h->n_pro = n_pro; h->n_anc = n_anc;
    const int L = plan.n_levels;
    if (n_pro == 0 || n_anc == 0 || L == 0) return GENPHI_OK;

    // parents as ranks (the planner checked that they exist and come first), leaves, relevance
    std::vector<int32_t> fa(n_ind, -1), mo(n_ind, -1);
    std::vector<char> has_child(n_ind, 0), rel(n_ind, 0);
    for (int64_t i = 0; i < n_ind; ++i) {
        if (father[i] != 0) { fa[i] = ranks.find(father[i]); has_child[fa[i]] = 1; }
        if (mother[i] != 0) { mo[i] = ranks.find(mother[i]); has_child[mo[i]] = 1; }
    }
    // one-hot columns of each ancestor rank: CSR over the ranks that are requested (columns ascending)
    std::vector<int32_t> oh_start(n_ind + 1, 0);
    for (int64_t j = 0; j < n_anc; ++j) oh_start[anc_rank[j] + 1]++;
    for (int64_t i = 0; i < n_ind; ++i) oh_start[i + 1] += oh_start[i];
    std::vector<int32_t> oh_of(n_anc);
    {
        std::vector<int32_t> fill(oh_start.begin(), oh_start.end() - 1);
        for (int64_t j = 0; j < n_anc; ++j) oh_of[fill[anc_rank[j]]++] = static_cast<int32_t>(j);
    }
    for (int64_t i = 0; i < n_ind; ++i)      // rank order: parents first
        rel[i] = oh_start[i + 1] > oh_start[i] || (fa[i] >= 0 && rel[fa[i]]) || (mo[i] >= 0 && rel[mo[i]]);

    // members of cut 0 (founders) by position, from the sources of cut 1 (every member of cut 0 is one of them)
    std::vector<int32_t> cut0(plan.cut_sizes[0], -1);
    if (L == 1) {
        for (int64_t k = 0; k < plan.cut_sizes[0]; ++k) cut0[k] = plan.final_members[k];
    } else {
        const genphi::LevelStep &st = plan.steps[0];
        const int32_t none = static_cast<int32_t>(st.n_prev);
        for (int64_t k = 0; k < st.n; ++k) {
            const int32_t o = st.ord[k];
            if (o >= 0) { cut0[st.srcA[k]] = o; continue; }
            const int32_t x = o & 0x7fffffff;
            if (st.srcA[k] != none) cut0[st.srcA[k]] = fa[x] >= 0 ? fa[x] : mo[x];
            if (st.srcB[k] != none) cut0[st.srcB[k]] = mo[x];
        }
    }
    // result row of each distinct proband (its first occurrence in pro_ids)
    std::vector<int32_t> out_row(n_ind, -1);
    for (int64_t k = n_pro - 1; k >= 0; --k) out_row[ranks.find(pro_ids[k])] = static_cast<int32_t>(k);

    auto add_item = [&](int32_t dst, int32_t A, int32_t B, int32_t x) {
        h->items.push_back(make_int4(dst, A, B, static_cast<int>(h->oh_cols.size())));
        for (int32_t q = oh_start[x]; q < oh_start[x + 1]; ++q) h->oh_cols.push_back(oh_of[q]);
        h->list_srcs.back() += (A >= 0) + (B >= 0);
    };
    auto open_list = [&](bool to_result) {
        h->list_begin.push_back(static_cast<int64_t>(h->items.size()));
        h->list_to_result.push_back(to_result);
        h->list_srcs.push_back(0.0);
    };
    auto close_list = [&]() { h->items.push_back(make_int4(-1, -1, -1, static_cast<int>(h->oh_cols.size()))); };
    auto emitted = [&](int32_t x) { return rel[x] && !has_child[x]; };

    // slots: a free list; slot_of_prev = slots of the members of the current source cut by position (-1 = zero row)
    std::vector<int32_t> free_slots;
    int32_t n_slots = 0;
    auto take = [&]() -> int32_t {
        if (!free_slots.empty()) { const int32_t s = free_slots.back(); free_slots.pop_back(); return s; }
        return n_slots++;
    };
    std::vector<int32_t> slot_prev(plan.cut_sizes[0], -1);
    open_list(L == 1);
    for (int64_t k = 0; k < plan.cut_sizes[0]; ++k) {
        const int32_t x = cut0[k];
        if (L == 1) {
            if (emitted(x)) add_item(out_row[x], -1, -1, x);
        } else if (rel[x]) {
            slot_prev[k] = take();
            add_item(slot_prev[k], -1, -1, x);
        }
    }
    close_list();
    std::vector<int32_t> rows;
    for (int s = 0; s + 1 < L; ++s) {
        const genphi::LevelStep &st = plan.steps[s];
        const bool last = s + 2 == L;
        const int32_t none = static_cast<int32_t>(st.n_prev);
        std::vector<int32_t> slot_cur(st.n, -1);
        std::vector<char> kept(st.n_prev, 0);
        rows.clear();
        for (int64_t k = 0; k < st.n; ++k) {
            const int32_t o = st.ord[k];
            if (o >= 0) { slot_cur[k] = slot_prev[st.srcA[k]]; kept[st.srcA[k]] = 1; continue; }   // dragged: same slot
            const int32_t x = o & 0x7fffffff;
            if (last ? emitted(x) : rel[x]) rows.push_back(static_cast<int32_t>(k));
        }
        genphi::reuse_order(st, rows);                        // siblings adjacent: the shared source row is served by L2
        open_list(last);
        for (int32_t k : rows) {
            const int32_t x = st.ord[k] & 0x7fffffff;
            const int32_t A = st.srcA[k] == none ? -1 : slot_prev[st.srcA[k]];
            const int32_t B = st.srcB[k] == none ? -1 : slot_prev[st.srcB[k]];
            if (last) { add_item(out_row[x], A, B, x); continue; }
            slot_cur[k] = take();
            add_item(slot_cur[k], A, B, x);
        }
        close_list();
        // members of the source cut that leave with this step: their slots serve the steps after it
        for (int64_t q = 0; q < st.n_prev; ++q)
            if (!kept[q] && slot_prev[q] >= 0) free_slots.push_back(slot_prev[q]);
        slot_prev.swap(slot_cur);
    }
    h->peak_slots = n_slots;                                  // (slots are taken from the free list first: the most ever live at once)
    h->list_begin.push_back(static_cast<int64_t>(h->items.size()));
    return GENPHI_OK;
}

int lanes_per_row(int C)
{
    const int pairs = (C + 1) / 2;
    int lpr = 1;
    while (lpr < pairs && lpr < 64) lpr *= 2;
    return lpr;
}

int compute_impl(genphi_gc *h, int32_t device)
{
    if (device < 0) GC_TRY(hipGetDevice(&device));
    if (h->device >= 0 && h->device != device) release_device(h);
    GC_TRY(hipSetDevice(device));
    h->device = device;
    h->computed = false;
    if (!h->stream) GC_TRY(genphi::cached_stream(&h->stream));
    const int64_t n_pro = h->n_pro, n_anc = h->n_anc;
    const size_t res_bytes = static_cast<size_t>(n_pro) * static_cast<size_t>(n_anc) * sizeof(float);
    size_t free_b = 0, total_b = 0;
    GC_TRY(hipMemGetInfo(&free_b, &total_b));
    const double usable = 0.9 * static_cast<double>(free_b + h->slot_bytes + (h->d_result ? res_bytes : 0));
    if (static_cast<double>(res_bytes) > usable)
        return genphi_set_error(GENPHI_ERR_ALLOC, "gen.gc: the result (" + std::to_string(res_bytes >> 20) + " MiB) does not fit on device " +
                                                      std::to_string(device));
    // panels: C columns each (GENPHI_GC_PANEL, else the default rule), G of them per launch (as many as the memory holds)
    const int64_t S = std::max<int64_t>(h->peak_slots, 1);
    const double slot_room = usable - static_cast<double>(res_bytes) -
                             16.0 * static_cast<double>(h->items.size()) - 4.0 * static_cast<double>(h->oh_cols.size()) - (64 << 20);
    int64_t C = h->panel_env > 0 ? h->panel_env : std::max<int64_t>(kPanelMinCols, static_cast<int64_t>(kPanelSlotBytes / (8.0 * S)));
    C = std::min(C, std::max<int64_t>(n_anc, 1));
    auto panel_bytes = [&](int64_t c) { return 8.0 * static_cast<double>(S) * static_cast<double>((c + 1) & ~int64_t(1)); };
    if (h->panel_env <= 0)
        while (C > 1 && panel_bytes(C) > slot_room) C = (C + 1) / 2;          // (more slot rows than the device holds at that width)
    if (panel_bytes(C) > slot_room)
        return genphi_set_error(GENPHI_ERR_ALLOC, "gen.gc: " + std::to_string(S) + " slots of " + std::to_string(C) +
                                                      " columns do not fit on device " + std::to_string(device) + " beside the result");
    const int64_t n_panels = n_anc > 0 ? (n_anc + C - 1) / C : 0;
    // panels per launch: one by default (see kPanelSlotBytes); with GENPHI_GC_PANEL as many as the memory holds, unless
    // GENPHI_GC_PANELS_PER_LAUNCH says otherwise (A/B and test hooks)
    int64_t G = 1;
    if (h->panel_env > 0) G = std::max<int64_t>(1, std::min<int64_t>(n_panels, static_cast<int64_t>(slot_room / panel_bytes(C))));
    if (h->group_env > 0) G = h->group_env;
    G = std::max<int64_t>(1, std::min<int64_t>({G, n_panels, 65535, static_cast<int64_t>(slot_room / panel_bytes(C))}));
    const int Cp = static_cast<int>((C + 1) & ~int64_t(1));
    const long long stride = static_cast<long long>(S) * Cp;
    const size_t need_slots = static_cast<size_t>(G) * static_cast<size_t>(stride) * sizeof(double);
    if (need_slots > h->slot_bytes) {
        (void)genphi::cached_free(h->d_slots);
        h->d_slots = nullptr; h->slot_bytes = 0;
        GC_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_slots), need_slots));
        h->slot_bytes = need_slots;
    }
    if (!h->d_result && res_bytes) GC_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_result), res_bytes));
    if (!h->d_items && !h->items.empty()) {
        GC_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_items), h->items.size() * sizeof(int4)));
        GC_TRY(hipMemcpyAsync(h->d_items, h->items.data(), h->items.size() * sizeof(int4), hipMemcpyHostToDevice, h->stream));
        if (!h->oh_cols.empty()) {
            GC_TRY(genphi::cached_malloc(reinterpret_cast<void **>(&h->d_oh), h->oh_cols.size() * sizeof(int)));
            GC_TRY(hipMemcpyAsync(h->d_oh, h->oh_cols.data(), h->oh_cols.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        }
    }
    h->panel_cols = static_cast<int32_t>(C);
    hipEvent_t e0, e1;
    GC_TRY(hipEventCreate(&e0));
    GC_TRY(hipEventCreate(&e1));
    GC_TRY(hipEventRecord(e0, h->stream));
    if (res_bytes) GC_TRY(hipMemsetAsync(h->d_result, 0, res_bytes, h->stream));
    const int lpr = lanes_per_row(static_cast<int>(C));
    const int rows_per_block = 4 * (64 / lpr);
    const int n_lists = static_cast<int>(h->list_to_result.size());
    double bytes = static_cast<double>(res_bytes);
    for (int64_t g0 = 0; g0 < n_panels; g0 += G) {
        const int64_t g = std::min<int64_t>(G, n_panels - g0);
        double cols = 0.0;                                     // columns of the panels of this launch
        for (int64_t p = g0; p < g0 + g; ++p) cols += static_cast<double>(std::min<int64_t>(C, n_anc - p * C));
        for (int k = 0; k < n_lists; ++k) {
            const int64_t b = h->list_begin[k], n_items = h->list_begin[k + 1] - 1 - b;
            if (n_items <= 0) continue;
            const bool to_res = h->list_to_result[k];
            bytes += cols * (8.0 * h->list_srcs[k] + (to_res ? 0.0 : 8.0 * static_cast<double>(n_items)));
            const dim3 grid(static_cast<unsigned>((n_items + rows_per_block - 1) / rows_per_block), static_cast<unsigned>(g));
            if (to_res)
                launch_step<true>(lpr, grid, h->stream, h->d_items + b, h->d_oh, static_cast<int>(n_items), h->d_slots, stride, Cp,
                                  static_cast<int>(C), static_cast<int>(n_anc), static_cast<int>(g0), h->d_result);
            else
                launch_step<false>(lpr, grid, h->stream, h->d_items + b, h->d_oh, static_cast<int>(n_items), h->d_slots, stride, Cp,
                                   static_cast<int>(C), static_cast<int>(n_anc), static_cast<int>(g0), h->d_result);
            GC_TRY(hipGetLastError());
        }
    }
    GC_TRY(hipEventRecord(e1, h->stream));
    GC_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    GC_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    h->sweep_ms = ms;
    h->alg_bytes = bytes;
    h->computed = true;
    return GENPHI_OK;
}

}  // namespace

extern "C" {

int genphi_gc_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                     const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, genphi_gc **out)
{
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_create: out is NULL");
    *out = nullptr;
    if (n_ind < 0 || n_pro < 0 || n_anc < 0 || (n_ind && (!ind || !father || !mother)) || (n_pro && !pro_ids) || (n_anc && !anc_ids))
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_create: bad sizes or NULL arrays");
    if (n_ind >= INT32_MAX || n_anc >= INT32_MAX || n_pro >= INT32_MAX)
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_create: more than 2^31 - 1 individuals, probands or ancestors");
    genphi_gc *h = new (std::nothrow) genphi_gc();
    if (!h) return genphi_set_error(GENPHI_ERR_ALLOC, "out of memory");
    if (const char *e = genphi::env_hook("GENPHI_GC_PANEL")) h->panel_env = std::max(0, std::atoi(e));
    if (const char *e = genphi::env_hook("GENPHI_GC_PANELS_PER_LAUNCH")) h->group_env = std::max(0, std::atoi(e));
    int rc;
    try {
        rc = plan_gc(h, n_ind, ind, father, mother, n_pro, pro_ids, n_anc, anc_ids);
    } catch (const std::bad_alloc &) { rc = genphi_set_error(GENPHI_ERR_ALLOC, "out of memory while planning gen.gc"); }
    if (rc) { delete h; return rc; }
    *out = h;
    return GENPHI_OK;
}

int genphi_gc_compute(genphi_gc *h, int32_t device)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_compute: NULL handle");
    if (h->n_pro == 0 || h->n_anc == 0) { h->computed = true; h->sweep_ms = 0.0; h->alg_bytes = 0.0; return GENPHI_OK; }
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, "gen.gc: no usable GPU");
    int rc;
    try {
        rc = compute_impl(h, device);
    } catch (const std::bad_alloc &) { rc = genphi_set_error(GENPHI_ERR_ALLOC, "out of host memory in gen.gc"); }
    (void)hipSetDevice(cur);
    return rc;
}

int genphi_gc_result_device(const genphi_gc *h, const float **d_ptr, int64_t *ld)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_result_device: nothing computed");
    if (d_ptr) *d_ptr = h->d_result;
    if (ld) *ld = h->n_anc;
    return GENPHI_OK;
}

int genphi_gc_result_to_host(genphi_gc *h, float *out)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_result_to_host: nothing computed");
    const size_t bytes = static_cast<size_t>(h->n_pro) * static_cast<size_t>(h->n_anc) * sizeof(float);
    if (!bytes) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_result_to_host: out is NULL");
    int cur = 0;
    GC_TRY(hipGetDevice(&cur));
    GC_TRY(hipSetDevice(h->device));
    const hipError_t e = hipMemcpyAsync(out, h->d_result, bytes, hipMemcpyDeviceToHost, h->stream);
    const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(h->stream) : e;
    (void)hipSetDevice(cur);
    if (e2 != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string("gen.gc result copy: ") + hipGetErrorString(e2));
    return GENPHI_OK;
}

int genphi_gc_stats(const genphi_gc *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *panel_cols)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, "genphi_gc_stats: NULL handle");
    if (sweep_ms) *sweep_ms = h->sweep_ms;
    if (algorithmic_bytes) *algorithmic_bytes = h->alg_bytes;
    if (peak_slots) *peak_slots = h->peak_slots;
    if (panel_cols) *panel_cols = h->panel_cols;
    return GENPHI_OK;
}

void genphi_gc_destroy(genphi_gc *h)
{
    if (!h) return;
    release_device(h);
    delete h;
}

}  // extern "C"
