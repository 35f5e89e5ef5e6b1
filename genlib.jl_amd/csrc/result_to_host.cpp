// result_to_host.cpp -- genphi_result_to_host and genphi_result_to_host_f64 (include/genphi.h): the resident result copied into the
// caller's array.  Host code around HIP API calls (pinned-ring workers, the mirror pass of the symmetric copy); no kernels.
#include <hip/hip_runtime.h>
#include <immintrin.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/genphi.h"
#include "devcache.h"
#include "planner.h"
#include "resident.h"

using genphi::ResidentView;

// tmp[q * nr + r] = src[r * w + q] for q < 16 and the first nr - nr % 8 rows r (genphi_result_to_host's mirror pass): 8 x 8
// transposes in AVX2 registers.  Returns the rows done.  (Host code of one function: the library is not built with -mavx2.)
__attribute__((target("avx2"))) static size_t mirror_gather16_avx2(const float *src, size_t w, size_t nr, float *tmp)
{
    size_t r = 0;
    for (; r + 8 <= nr; r += 8) {
        for (int h = 0; h < 2; ++h) {                       // columns [8 h, 8 h + 8)
            __m256 v[8];
            for (int k = 0; k < 8; ++k) v[k] = _mm256_loadu_ps(src + (r + k) * w + 8 * h);
            const __m256 t0 = _mm256_unpacklo_ps(v[0], v[1]), t1 = _mm256_unpackhi_ps(v[0], v[1]);
            const __m256 t2 = _mm256_unpacklo_ps(v[2], v[3]), t3 = _mm256_unpackhi_ps(v[2], v[3]);
            const __m256 t4 = _mm256_unpacklo_ps(v[4], v[5]), t5 = _mm256_unpackhi_ps(v[4], v[5]);
            const __m256 t6 = _mm256_unpacklo_ps(v[6], v[7]), t7 = _mm256_unpackhi_ps(v[6], v[7]);
            const __m256 u0 = _mm256_shuffle_ps(t0, t2, 0x44), u1 = _mm256_shuffle_ps(t0, t2, 0xee);
            const __m256 u2 = _mm256_shuffle_ps(t1, t3, 0x44), u3 = _mm256_shuffle_ps(t1, t3, 0xee);
            const __m256 u4 = _mm256_shuffle_ps(t4, t6, 0x44), u5 = _mm256_shuffle_ps(t4, t6, 0xee);
            const __m256 u6 = _mm256_shuffle_ps(t5, t7, 0x44), u7 = _mm256_shuffle_ps(t5, t7, 0xee);
            _mm256_storeu_ps(tmp + (8 * h + 0) * nr + r, _mm256_permute2f128_ps(u0, u4, 0x20));
            _mm256_storeu_ps(tmp + (8 * h + 1) * nr + r, _mm256_permute2f128_ps(u1, u5, 0x20));
            _mm256_storeu_ps(tmp + (8 * h + 2) * nr + r, _mm256_permute2f128_ps(u2, u6, 0x20));
            _mm256_storeu_ps(tmp + (8 * h + 3) * nr + r, _mm256_permute2f128_ps(u3, u7, 0x20));
            _mm256_storeu_ps(tmp + (8 * h + 4) * nr + r, _mm256_permute2f128_ps(u0, u4, 0x31));
            _mm256_storeu_ps(tmp + (8 * h + 5) * nr + r, _mm256_permute2f128_ps(u1, u5, 0x31));
            _mm256_storeu_ps(tmp + (8 * h + 6) * nr + r, _mm256_permute2f128_ps(u2, u6, 0x31));
            _mm256_storeu_ps(tmp + (8 * h + 7) * nr + r, _mm256_permute2f128_ps(u3, u7, 0x31));
        }
    }
    return r;
}

extern "C" {

int genphi_result_to_host_f64(genphi_plan *p, double *out)
{
    if (!p) return genphi_set_error(GENPHI_ERR_ARG, "plan is NULL");
    const ResidentView v = genphi::resident_view(p);
    if (v.n_rows == 0 || v.n_pro == 0) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "out is NULL");
    if (!v.res_f64 || !v.on_device || !v.result64)
        return genphi_set_error(GENPHI_ERR_ARG, "no resident Float64 result: call genphi_compute_device with GENPHI_FLAG_STORAGE_F64 first");
    GENPHI_RESIDENT_TRY("hipSetDevice(p->device)", hipSetDevice(v.device));
    const size_t N = static_cast<size_t>(v.n_pro);
    GENPHI_RESIDENT_TRY("hipMemcpy2D(out, N * sizeof(double), p->result64, static_cast<size_t>(p->res_ld) * sizeof(double), N * sizeof(double), static_cast<size_t>(p->res_n_rows), hipMemcpyDeviceToHost)",
                        hipMemcpy2D(out, N * sizeof(double), v.result64, static_cast<size_t>(v.ld) * sizeof(double), N * sizeof(double),
                                    static_cast<size_t>(v.n_rows), hipMemcpyDeviceToHost));
    return GENPHI_OK;
}

int genphi_result_to_host(genphi_plan *p, float *out)
{
    if (!p) return genphi_set_error(GENPHI_ERR_ARG, "plan is NULL");
    const ResidentView v = genphi::resident_view(p);
    if (v.n_rows == 0 || v.n_pro == 0) return GENPHI_OK;
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, "out is NULL");
    if (v.res_f64) {
        // Float64 sweep: deliver RN32 of the Float64 values (ONE rounding, like gen.f, src/compute.jl:500-511)
        const size_t n = static_cast<size_t>(v.n_rows) * static_cast<size_t>(v.n_pro);
        std::vector<double> tmp(n);
        const int rc = genphi_result_to_host_f64(p, tmp.data());
        if (rc) return rc;
        for (size_t k = 0; k < n; ++k) out[k] = static_cast<float>(tmp[k]);
        return GENPHI_OK;
    }
    if (!v.on_device || !v.result) return genphi_set_error(GENPHI_ERR_DEVICE, "no resident result: call genphi_compute_device first");
    GENPHI_RESIDENT_TRY("hipSetDevice(p->device)", hipSetDevice(v.device));
    const size_t N = static_cast<size_t>(v.n_pro);
    const size_t rows = static_cast<size_t>(v.n_rows);
    GENPHI_RESIDENT_TRY("hipStreamSynchronize(p->stream)", hipStreamSynchronize(v.stream));
    // Large results go through a ring of pinned staging buffers: every worker thread owns a
    // stream and two pinned chunks, the DMA engine fills one chunk (device pitch -> dense rows)
    // while the thread copies the other into the caller's pageable array.  A plain hipMemcpy2D
    // into pageable memory is staged by the runtime on ONE thread (~17 GB/s; 23 GB/s with 8
    // concurrent calls); the PCIe Gen5 link carries more than twice that.
    const size_t bytes = rows * N * sizeof(float);
    // A FULL result is bit-symmetric (every level is: both (i, j) and (j, i) are the same Float64 expression), and the plain copy is
    // bound by the PCIe link (55 GB/s into warm pages, 53 with first-touch page faults), so GENPHI_D2H_SYM=1 sends only the tiles on and
    // above the diagonal across the link and lets the worker threads mirror them into the lower triangle on the host.  OPT-IN: measured
    // at 1e5 probands (profiles/microbench/out/r04_d2h_symmetric_vs_plain_cfg4.out) it takes 440-1140 ms warm and 615-1420 ms into fresh
    // pages against a steady 724 / 756 ms for the plain copy -- the mirror pass makes the HOST the bottleneck, and a GPU box gives the
    // process 16 CPUs (cgroup quota): whenever the 16 workers, the Python thread and the runtime's helpers exceed it, the kernel throttles
    // the lot.  On a host with cores to spare it is the faster path; here it is not reliably so, hence not the default.
    bool sym = rows == N && v.row_begin == 0 && N >= 2 && !v.tun->d2h_pageable && v.tun->d2h_sym == 1;
    int n_thr = 1;
    if (bytes >= (size_t(64) << 20) || sym) {              // (one worker per 32 MB up to 8: the ring is kept between calls, so mid-size results use it too)
        n_thr = sym ? 16 : static_cast<int>(std::min<size_t>(8, bytes >> 25));
        if (v.tun->d2h_threads > 0) n_thr = std::max(1, std::min(32, v.tun->d2h_threads));
    }
    const size_t row_bytes = N * sizeof(float);
    const size_t tile_r = v.tun->d2h_tile_rows > 0 ? static_cast<size_t>(v.tun->d2h_tile_rows) : 256;
    const size_t tile_c = v.tun->d2h_tile_cols > 0 ? static_cast<size_t>(v.tun->d2h_tile_cols) : 8192;
    // (16 MB chunks; 4 MB for results below 2 GB, whose workers have only a few chunks each to overlap the DMA with the host copy)
    const size_t chunk_mb = v.tun->d2h_chunk_mb > 0 ? static_cast<size_t>(v.tun->d2h_chunk_mb) : (bytes < (size_t(2) << 30) ? 4 : 16);
    const size_t chunk_rows = std::max<size_t>(1, (chunk_mb << 20) / row_bytes);
    const size_t chunk_bytes = sym ? std::max<size_t>(tile_r * std::min(tile_c, N) * sizeof(float), 4096) : chunk_rows * row_bytes;
    bool pinned = (n_thr > 1 || sym) && !v.tun->d2h_pageable;
    // (the ring belongs to the device, not to the plan: pinning 256 MB costs 60-100 ms and unpinning them 80 ms -- per one-shot call
    // when every plan had its own; devcache.h)
    genphi::PinnedRing *ring = nullptr;
    std::unique_lock<std::mutex> ring_lock;
    if (pinned) {
        ring = &genphi::pinned_ring(v.device);
        ring_lock = std::unique_lock<std::mutex>(ring->mu);
        if (!genphi::pinned_ring_reserve(*ring, static_cast<size_t>(2 * n_thr), chunk_bytes, static_cast<size_t>(n_thr))) {
            pinned = false;                             // could not pin: fall back to direct copies
            ring_lock.unlock();
            ring = nullptr;
        }
    }
    if (!pinned) sym = false;
    std::vector<hipError_t> errs(n_thr, hipSuccess);
    if (sym) {
        // items: (row block I, column tile J) with the tile's columns clipped to [max(c0, a), c1): on or right of the diagonal block
        struct Item { uint32_t a, b, cs, c1; };
        std::vector<Item> items;
        for (size_t a = 0; a < N; a += tile_r) {
            const size_t b = std::min(N, a + tile_r);
            for (size_t c0 = a / tile_c * tile_c; c0 < N; c0 += tile_c) {
                const size_t cs = std::max(c0, a), c1 = std::min(N, c0 + tile_c);
                items.push_back({static_cast<uint32_t>(a), static_cast<uint32_t>(b), static_cast<uint32_t>(cs), static_cast<uint32_t>(c1)});
            }
        }
        std::atomic<size_t> next{0};
        const size_t src_pitch = static_cast<size_t>(v.ld) * sizeof(float);
        const bool avx2 = __builtin_cpu_supports("avx2") != 0;
        auto worker = [&](int t) {
            hipError_t e = hipSetDevice(v.device);
            if (e != hipSuccess) { errs[t] = e; return; }
            hipStream_t st = ring->stream[t];
            float *pb[2] = {static_cast<float *>(ring->chunk[2 * t]), static_cast<float *>(ring->chunk[2 * t + 1])};
            auto issue = [&](const Item &it, float *dst) {
                const size_t w = it.c1 - it.cs;
                return hipMemcpy2DAsync(dst, w * sizeof(float), v.result + static_cast<size_t>(it.a) * static_cast<size_t>(v.ld) + it.cs, src_pitch,
                                        w * sizeof(float), it.b - it.a, hipMemcpyDeviceToHost, st);
            };
            // (waits sleep instead of spinning -- a blocking-sync event per buffer: the host side is the bottleneck of this copy,
            // and a GPU box gives a process 16 CPUs; spinning waiters take them from the threads that mirror tiles)
            hipEvent_t evb[2] = {nullptr, nullptr};
            for (hipEvent_t &x : evb)
                if ((e = hipEventCreateWithFlags(&x, hipEventBlockingSync | hipEventDisableTiming)) != hipSuccess) { errs[t] = e; return; }
            size_t cur = next.fetch_add(1);
            if (cur >= items.size()) { for (hipEvent_t x : evb) (void)hipEventDestroy(x); return; }
            e = issue(items[cur], pb[0]);
            if (e == hipSuccess) e = hipEventRecord(evb[0], st);
            for (int k = 0; e == hipSuccess; ++k) {
                e = hipEventSynchronize(evb[k & 1]);        // item `cur` has landed in pb[k & 1]
                if (e != hipSuccess) break;
                const size_t nxt = next.fetch_add(1);
                if (nxt < items.size()) {                   // the DMA engine fills the other buffer meanwhile
                    e = issue(items[nxt], pb[(k + 1) & 1]);
                    if (e == hipSuccess) e = hipEventRecord(evb[(k + 1) & 1], st);
                }
                const Item it = items[cur];
                const float *blk = pb[k & 1];
                const size_t w = it.c1 - it.cs, nr = it.b - it.a;
                for (size_t r = 0; r < nr; ++r)             // the tile itself
                    std::memcpy(out + (it.a + r) * N + it.cs, blk + r * w, w * sizeof(float));
                // its mirror image: columns right of the diagonal block become the rows' entries [a, b), 16 columns (a cache
                // line of every tile row) at a time through a small buffer, written as runs of nr floats
                const size_t ts = std::max<size_t>(it.cs, it.b);
                constexpr size_t KB = 16;
                static thread_local std::vector<float> tmp;
                tmp.resize(KB * nr);
                for (size_t cb0 = ts; cb0 < it.c1; cb0 += KB) {
                    const size_t nb = std::min(KB, it.c1 - cb0);
                    const float *src = blk + (cb0 - it.cs);
                    if (nb == KB) {
                        size_t r = 0;
                        if (avx2) r = mirror_gather16_avx2(src, w, nr, tmp.data());       // 8 x 8 register transposes, whole multiples of 8 rows
                        for (; r < nr; ++r) {
                            const float *sr = src + r * w;
#pragma unroll
                            for (size_t q = 0; q < KB; ++q) tmp[q * nr + r] = sr[q];
                        }
                    } else {
                        for (size_t r = 0; r < nr; ++r)
                            for (size_t q = 0; q < nb; ++q) tmp[q * nr + r] = src[r * w + q];
                    }
                    for (size_t q = 0; q < nb; ++q) std::memcpy(out + (cb0 + q) * N + it.a, tmp.data() + q * nr, nr * sizeof(float));
                }
                if (nxt >= items.size()) break;
                cur = nxt;
            }
            for (hipEvent_t x : evb) (void)hipEventDestroy(x);
            errs[t] = e;
        };
        std::vector<std::thread> th;
        for (int t = 0; t < n_thr; ++t) th.emplace_back(worker, t);
        for (auto &x : th) x.join();
        for (hipError_t e : errs)
            if (e != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string("genphi_result_to_host: ") + hipGetErrorString(e));
        return GENPHI_OK;
    }
    const bool d2h_stats = genphi::env_hook("GENPHI_D2H_STATS") != nullptr;
    auto copy_block = [&](int t) {
        const size_t r0 = rows * t / n_thr, r1 = rows * (t + 1) / n_thr;
        if (r1 == r0) return;
        hipError_t e = hipSetDevice(v.device);
        if (e != hipSuccess) { errs[t] = e; return; }
        const size_t src_pitch = static_cast<size_t>(v.ld) * sizeof(float);
        if (!pinned) {
            errs[t] = hipMemcpy2D(out + r0 * N, row_bytes, v.result + r0 * static_cast<size_t>(v.ld), src_pitch,
                                  row_bytes, r1 - r0, hipMemcpyDeviceToHost);
            return;
        }
        hipStream_t st = ring->stream[t];
        char *pb[2] = {static_cast<char *>(ring->chunk[2 * t]), static_cast<char *>(ring->chunk[2 * t + 1])};
        const size_t n_chunks = (r1 - r0 + chunk_rows - 1) / chunk_rows;
        auto issue = [&](size_t c) {
            const size_t a = r0 + c * chunk_rows, b = std::min(r1, a + chunk_rows);
            return hipMemcpy2DAsync(pb[c & 1], row_bytes, v.result + a * static_cast<size_t>(v.ld), src_pitch,
                                    row_bytes, b - a, hipMemcpyDeviceToHost, st);
        };
        e = issue(0);
        double t_wait = 0.0, t_host = 0.0;
        auto clk = [] { return std::chrono::steady_clock::now(); };
        for (size_t c = 0; c < n_chunks && e == hipSuccess; ++c) {
            const auto t0 = clk();
            e = hipStreamSynchronize(st);               // chunk c has landed in pb[c & 1]
            if (e != hipSuccess) break;
            if (c + 1 < n_chunks) e = issue(c + 1);     // the DMA engine fills the other buffer meanwhile
            const auto t1 = clk();
            const size_t a = r0 + c * chunk_rows, b = std::min(r1, a + chunk_rows);
            std::memcpy(out + a * N, pb[c & 1], (b - a) * row_bytes);
            if (d2h_stats) { t_wait += std::chrono::duration<double, std::milli>(t1 - t0).count(); t_host += std::chrono::duration<double, std::milli>(clk() - t1).count(); }
        }
        if (d2h_stats) std::fprintf(stderr, "[genphi d2h] thread %d: %zu chunks, waiting for the DMA %.2f ms, copying into the caller's array %.2f ms\n", t, n_chunks, t_wait, t_host);
        errs[t] = e;
    };
    if (n_thr == 1) copy_block(0);
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < n_thr; ++t) th.emplace_back(copy_block, t);
        for (auto &x : th) x.join();
    }
    for (hipError_t e : errs)
        if (e != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string("genphi_result_to_host: ") + hipGetErrorString(e));
    return GENPHI_OK;
}

}  // extern "C"
