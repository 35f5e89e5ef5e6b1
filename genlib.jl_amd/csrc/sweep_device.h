// sweep_device.h -- the device side of a sweep handle that the ten sweep files (gc, occ, dist, depth, completeness, implex, simu, ident, link, retain) share:
// everything around the kernels that does not depend on the arithmetic.  A sweep's file keeps its kernels, its handle's own
// fields, its PanelRule, the allocation and pre-fill of its result, its launch callable, its extra passes and its extern "C"
// functions.  The four gene-dropping sweeps share more on top of this: drop_host.h, and the three label sweeps
// label_sweep.h.  Host functions only; every including file gets its own copy (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "../../include/genphi.h"
#include "ancestor_sweep.h"
#include "devbuf.h"
#include "devcache.h"
#include "planner.h"
#include "sweep_panels.h"
#include "error.h"

#define GENPHI_HIP_TRY(expr)                                                                                    \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// CALL with LPR = lpr as a constant: the lanes-per-row instantiations of a kernel
#define GENPHI_LPR_SWITCH(lpr, CALL)                   \
    switch (lpr) {                                     \
    case 1: { constexpr int LPR = 1; CALL; } break;    \
    case 2: { constexpr int LPR = 2; CALL; } break;    \
    case 4: { constexpr int LPR = 4; CALL; } break;    \
    case 8: { constexpr int LPR = 8; CALL; } break;    \
    case 16: { constexpr int LPR = 16; CALL; } break;  \
    case 32: { constexpr int LPR = 32; CALL; } break;  \
    default: { constexpr int LPR = 64; CALL; } break;  \
    }

namespace {

// Lanes per row: the power of two >= the 16-byte vectors (completeness: the columns) of a row, at most a wave.
inline int lanes_per_row(int vectors)
{
    int lpr = 1;
    while (lpr < vectors && lpr < 64) lpr *= 2;
    return lpr;
}

// a test or A/B hook that holds a count (0 = not set)
inline int32_t hook_count(const char *name)
{
    const char *e = genphi::env_hook(name);
    return e ? std::max(0, std::atoi(e)) : 0;
}

template <typename T, typename V>
void put(T *dst, V value)
{
    if (dst) *dst = static_cast<T>(value);
}

// Restores the caller's current device.
struct DeviceGuard {
    int cur = 0;
    hipError_t err;
    DeviceGuard() : err(hipGetDevice(&cur)) {}
    ~DeviceGuard() { if (err == hipSuccess) (void)hipSetDevice(cur); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

using genphi::DevBuf;

// What every sweep handle holds on a device.  Its device blocks are DevBufs (devbuf.h): d_slots here and the handle's own members,
// which it registers (own).  release() gives them all back on the handle's device, held_bytes() sums them.
// A handle is deleted only by destroy_entry, after release(), or by create_entry before anything is allocated: the destructor of a
// DevBuf never has a block left to free, so it never frees under a current device that is not the block's.
struct SweepDevice {
    int device = -1;
    hipStream_t stream = nullptr;
    DevBuf<char> d_slots;                    // the slot rows (implex: the frontier rows), grown on demand
    bool computed = false;
    double sweep_ms = 0.0, alg_bytes = 0.0;
    int64_t n_launches = 0;
    static constexpr int kMaxBlocks = 12;
    genphi::DevBlock *blocks[kMaxBlocks] = {&d_slots};
    int n_blocks = 1;

    SweepDevice() = default;
    SweepDevice(const SweepDevice &) = delete;
    SweepDevice &operator=(const SweepDevice &) = delete;

    // Called from the handle's constructor, and from that of a base handle that has blocks of its own (label_sweep.h): a call is bounded
    // when it is compiled, the calls together when the first handle of the type is created.
    template <typename... T>
    void own(DevBuf<T> &...bufs)
    {
        static_assert(sizeof...(T) < kMaxBlocks, "more blocks than the list holds");
        if (n_blocks + static_cast<int>(sizeof...(T)) > kMaxBlocks) std::abort();
        ((blocks[n_blocks++] = &bufs), ...);
    }

    template <typename T>
    T *slots() const { return reinterpret_cast<T *>(d_slots.get()); }

    // the handle's own blocks, beside the slot rows
    size_t held_bytes() const
    {
        size_t sum = 0;
        for (int i = 1; i < n_blocks; ++i) sum += blocks[i]->bytes();
        return sum;
    }

    void release()
    {
        if (device < 0) return;
        DeviceGuard keep;
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (int i = 0; i < n_blocks; ++i) blocks[i]->release();
        if (stream) genphi::cached_stream_release(stream, device);
        stream = nullptr;
        device = -1;
        computed = false;
    }

    // The opening of a compute: the device (-1: the current one), what another device holds released, the cached stream.
    int select(int32_t dev)
    {
        if (dev < 0) GENPHI_HIP_TRY(hipGetDevice(&dev));
        if (device >= 0 && device != dev) release();
        GENPHI_HIP_TRY(hipSetDevice(dev));
        device = dev;
        computed = false;
        if (!stream) GENPHI_HIP_TRY(genphi::cached_stream(&stream));
        return GENPHI_OK;
    }

    // 90% of what is free or held by this handle already
    int usable_bytes(double &usable, size_t held) const
    {
        size_t free_b = 0, total_b = 0;
        GENPHI_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        usable = 0.9 * static_cast<double>(free_b + d_slots.bytes() + held);
        return GENPHI_OK;
    }

    // The panels of a sweep over n_cols columns beside a result of res_bytes (res_held: allocated already), and their slot rows.
    int size_panels(genphi::PanelLayout &L, const genphi::PanelRule &rule, const genphi::SweepSchedule &s, int64_t n_cols, int32_t panel_env,
                    int32_t group_env, size_t res_bytes, bool res_held, const std::string &who)
    {
        double usable = 0.0;
        if (int rc = usable_bytes(usable, res_held ? res_bytes : 0)) return rc;
        if (static_cast<double>(res_bytes) > usable)
            return genphi_set_error(GENPHI_ERR_ALLOC, who + ": the result (" + std::to_string(res_bytes >> 20) + " MiB) does not fit on device " +
                                                          std::to_string(device));
        const double slot_room = usable - static_cast<double>(res_bytes) - 16.0 * static_cast<double>(s.items.size()) -
                                 4.0 * static_cast<double>(s.oh_cols.size() + s.pro_slots.size()) - (64 << 20);
        if (genphi::plan_panels(L, rule, s.peak_slots, n_cols, panel_env, group_env, slot_room))
            return genphi_set_error(GENPHI_ERR_ALLOC, who + ": " + std::to_string(L.slots) + " slots of " + std::to_string(L.C) +
                                                          " columns do not fit on device " + std::to_string(device) + " beside the result");
        GENPHI_HIP_TRY(d_slots.reserve(L.slot_bytes));
        return GENPHI_OK;
    }

    // a list of the plan, uploaded once; an empty list stays a null pointer (D and S of one size: int4 for SweepItem)
    template <typename D, typename S>
    int upload(DevBuf<D> &dst, const std::vector<S> &src)
    {
        static_assert(sizeof(D) == sizeof(S), "uploaded as it is");
        if (dst.get() || src.empty()) return GENPHI_OK;
        GENPHI_HIP_TRY(dst.reserve(src.size()));
        GENPHI_HIP_TRY(hipMemcpyAsync(dst.get(), src.data(), dst.bytes(), hipMemcpyHostToDevice, stream));
        return GENPHI_OK;
    }

    // f() on the handle's device and stream; what: the head of the error text
    template <typename F>
    int on_device(const std::string &what, F &&f)
    {
        DeviceGuard keep;
        GENPHI_HIP_TRY(keep.err);
        GENPHI_HIP_TRY(hipSetDevice(device));
        const hipError_t e = f();
        if (e != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, what + ": " + hipGetErrorString(e));
        return GENPHI_OK;
    }

    // bytes from the device (src) to the host
    int copy_out(void *out, const void *src, size_t bytes, const std::string &who)
    {
        return on_device(who + " result copy", [&] {
            const hipError_t e = hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, stream);
            return e == hipSuccess ? hipStreamSynchronize(stream) : e;
        });
    }

    // rows of width bytes at a pitch of src_pitch bytes, packed on the host
    int copy_out_2d(void *out, const void *src, size_t src_pitch, size_t width, size_t rows, const std::string &who)
    {
        return on_device(who + " result copy", [&] {
            const hipError_t e = hipMemcpy2DAsync(out, width, src, src_pitch, width, rows, hipMemcpyDeviceToHost, stream);
            return e == hipSuccess ? hipStreamSynchronize(stream) : e;
        });
    }

    void stats(double *ms, double *algorithmic_bytes, int64_t *launches) const
    {
        put(ms, sweep_ms);
        put(algorithmic_bytes, alg_bytes);
        put(launches, n_launches);
    }
};

// One timed sweep: the event pair around it (destroyed on every path) and the bytes and launches it counts.
struct SweepRun {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double bytes = 0.0;
    int64_t launches = 0;
    SweepRun() = default;
    SweepRun(const SweepRun &) = delete;
    SweepRun &operator=(const SweepRun &) = delete;
    ~SweepRun()
    {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    int begin(SweepDevice &d, double result_bytes)
    {
        GENPHI_HIP_TRY(hipEventCreate(&e0));
        GENPHI_HIP_TRY(hipEventCreate(&e1));
        GENPHI_HIP_TRY(hipEventRecord(e0, d.stream));
        bytes = result_bytes;
        return GENPHI_OK;
    }
    int end(SweepDevice &d)
    {
        GENPHI_HIP_TRY(hipEventRecord(e1, d.stream));
        GENPHI_HIP_TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        GENPHI_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        d.sweep_ms = ms;
        d.alg_bytes = bytes;
        d.n_launches = launches;
        d.computed = true;
        return GENPHI_OK;
    }
};

// One launch of the loop below: a list of items over the panels [panel0, panel0 + grid.y).
struct ListLaunch {
    const int4 *items;
    int n_items;
    bool to_result;
    dim3 grid;
    int panel0;
};

// The sweep: for every group of L.per_launch panels, every list of the schedule in order, then after(panel0, panels, row_bytes)
// (a pass over the group's slot rows; nonzero ends the sweep).  A block computes rows_per_block rows; the list that goes to the
// result is launched over units of result_rows items (a kernel that reduces them; else 1).  Counts launches and algorithmic bytes.
template <typename Launch, typename After>
int sweep_lists(SweepRun &run, const genphi::SweepSchedule &s, const int4 *d_items, const genphi::PanelRule &rule, const genphi::PanelLayout &L,
                int64_t n_cols, int rows_per_block, int result_rows, Launch &&launch, After &&after)
{
    const int n_lists = static_cast<int>(s.list_to_result.size());
    for (int64_t g0 = 0; g0 < L.n_panels; g0 += L.per_launch) {
        const int64_t g = std::min<int64_t>(L.per_launch, L.n_panels - g0);
        const double row_bytes = L.row_bytes(rule, n_cols, g0, g);
        for (int k = 0; k < n_lists; ++k) {
            const int64_t b = s.list_begin[k], n_items = s.list_begin[k + 1] - 1 - b;
            if (n_items <= 0) continue;
            const bool to_res = s.list_to_result[k];
            run.bytes += row_bytes * (s.list_srcs[k] + (to_res ? 0.0 : static_cast<double>(n_items)));
            const int64_t units = to_res ? (n_items + result_rows - 1) / result_rows : n_items;
            launch(ListLaunch{d_items + b, static_cast<int>(n_items), to_res,
                              dim3(static_cast<unsigned>((units + rows_per_block - 1) / rows_per_block), static_cast<unsigned>(g)), static_cast<int>(g0)});
            GENPHI_HIP_TRY(hipGetLastError());
            ++run.launches;
        }
        if (int rc = after(g0, g, row_bytes)) return rc;
    }
    return GENPHI_OK;
}

template <typename Launch>
int sweep_lists(SweepRun &run, const genphi::SweepSchedule &s, const int4 *d_items, const genphi::PanelRule &rule, const genphi::PanelLayout &L,
                int64_t n_cols, int rows_per_block, int result_rows, Launch &&launch)
{
    return sweep_lists(run, s, d_items, rule, L, n_cols, rows_per_block, result_rows, launch, [](int64_t, int64_t, double) { return 0; });
}

// max_anc: the entry point's limit on n_anc (0: it takes no ancestors)
inline int check_create_args(const char *fn, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                             const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, const void *out, int64_t max_anc)
{
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, std::string(fn) + ": out is NULL");
    if (n_ind < 0 || n_pro < 0 || n_anc < 0 || (n_ind && (!ind || !father || !mother)) || (n_pro && !pro_ids) || (n_anc && !anc_ids))
        return genphi_set_error(GENPHI_ERR_ARG, std::string(fn) + ": bad sizes or NULL arrays");
    if (n_ind >= INT32_MAX || n_pro >= INT32_MAX || (max_anc && n_anc >= max_anc))
        return genphi_set_error(GENPHI_ERR_ARG, std::string(fn) + (max_anc ? ": more than 2^31 - " + std::to_string(int64_t(INT32_MAX) + 1 - max_anc) +
                                                                                 " individuals, probands or ancestors"
                                                                           : ": more than 2^31 - 2 individuals or probands"));
    return GENPHI_OK;
}

// After the argument checks: a new handle, planned on the host by plan(h); who: "gen.gc", ..
template <typename H, typename Plan>
int create_entry(H **out, const char *who, Plan &&plan)
{
    H *h = new (std::nothrow) H();
    if (!h) return genphi_set_error(GENPHI_ERR_ALLOC, "out of memory");
    int rc;
    try {
        rc = plan(h);
    } catch (const std::bad_alloc &) { rc = genphi_set_error(GENPHI_ERR_ALLOC, std::string("out of memory while planning ") + who); }
    if (rc) { delete h; return rc; }
    *out = h;
    return GENPHI_OK;
}

// impl(h, device) with the caller's current device restored; an empty handle (h->empty()) has nothing to compute.
template <typename H, typename Impl>
int compute_entry(H *h, int32_t device, const char *fn, const char *who, Impl &&impl)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, std::string(fn) + ": NULL handle");
    if (h->empty()) { h->computed = true; h->sweep_ms = 0.0; h->alg_bytes = 0.0; h->n_launches = 0; return GENPHI_OK; }
    DeviceGuard keep;
    if (keep.err != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(who) + ": no usable GPU");
    try {
        return impl(h, device);
    } catch (const std::bad_alloc &) { return genphi_set_error(GENPHI_ERR_ALLOC, std::string("out of host memory in ") + who); }
}

template <typename H>
void destroy_entry(H *h)
{
    if (!h) return;
    h->release();
    delete h;
}

}  // namespace
