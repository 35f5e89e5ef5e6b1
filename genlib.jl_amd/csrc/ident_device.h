// ident_device.h -- the label sweep of gen.simuIdentity that gen.simuRetention shares (ident.hip, retain.hip): the init kernel of the
// constant sides and the step kernel of one level, on the row layout at the head of ident.hip: row r, pair j, side s, plane b at
// ((r * Pn + j) * 2 + s) * B + b, 16-byte elements.  link.hip keeps its own variants over (simulation, locus).  Every including file
// gets its own copy (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>

#include "drop_device.h"

namespace {

// The constant sides: a thread per (label, pair of words) writes the B planes of the side that carries the label.
__global__ void __launch_bounds__(256)
ident_init_kernel(const long long *__restrict__ const_side, long long n_labels, ulonglong2 *__restrict__ rows, int Pn, int Pc, int B)
{
    const long long t = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const long long k = t / Pc;
    if (k >= n_labels) return;
    const int c = static_cast<int>(t % Pc);
    const long long side = const_side[k];                // 2 * row + side
    ulonglong2 *dst = rows + ((side >> 1) * Pn + c) * 2 * B + (side & 1) * B;
    for (int b = 0; b < B; ++b) {
        const u64 v = (k >> b) & 1 ? ~0ull : 0ull;
        dst[b] = make_ulonglong2(v, v);
    }
}

// One level: row row0 + r from the rows of its parents (simu_step_kernel's lanes: LPR lanes per row, lane l owns the pairs l,
// l + LPR, .. < Pc; a wave holds 64 / LPR rows).  A parent row < 0 is a constant side: the init kernel wrote it.  rows is read
// (earlier levels) and written (this level): no __restrict__.
template <int LPR>
__global__ void __launch_bounds__(256)
ident_step_kernel(const int *__restrict__ fa_row, const int *__restrict__ mo_row, const long long *__restrict__ ids, int n_rows,
                  long long row0, ulonglong2 *rows, int Pn, int Pc, int B, unsigned first_pair, unsigned k0, unsigned k1)
{
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = (static_cast<long long>(blockIdx.x) * 4 + wave) * RPW + lane / LPR;
    if (r >= n_rows) return;
    const int l = lane % LPR;
    const int f = fa_row[r], m = mo_row[r];
    const u64 id = static_cast<u64>(ids[r]);
    const unsigned id_lo = static_cast<unsigned>(id), id_hi = static_cast<unsigned>(id >> 32);
    const long long B2 = 2 * B;
    const ulonglong2 *fs = rows + static_cast<long long>(f < 0 ? 0 : f) * Pn * B2;
    const ulonglong2 *ms = rows + static_cast<long long>(m < 0 ? 0 : m) * Pn * B2;
    ulonglong2 *dst = rows + (row0 + r) * Pn * B2;
    for (int c = l; c < Pc; c += LPR) {
        if (f >= 0) {
            const ulonglong2 T = philox_pair(id_lo, id_hi, first_pair + static_cast<unsigned>(c), 0u, k0, k1);
            const ulonglong2 *src = fs + c * B2;
            ulonglong2 *out = dst + c * B2;
            for (int b = 0; b < B; ++b) {
                const ulonglong2 p = src[b], q = src[B + b];
                out[b] = meiosis(T, p, q);
            }
        }
        if (m >= 0) {
            const ulonglong2 T = philox_pair(id_lo, id_hi, first_pair + static_cast<unsigned>(c), 1u, k0, k1);
            const ulonglong2 *src = ms + c * B2;
            ulonglong2 *out = dst + c * B2 + B;
            for (int b = 0; b < B; ++b) {
                const ulonglong2 p = src[b], q = src[B + b];
                out[b] = meiosis(T, p, q);
            }
        }
    }
}

}  // namespace
