// drop_device.h -- the device helpers the four gene-dropping sweeps (simu.hip, ident.hip, retain.hip, link.hip) share: the random word
// of a meiosis, the meiosis itself and the mask of the simulated columns (link.hip: of the loci).  gen.simuIdentity relies on drawing
// THE word gen.simuSample draws for the same (seed, ID, side, absolute pair index): both take it from here.  The host side of the four
// handles is drop_host.h; the label sweep of the last three is label_sweep.h.
#pragma once
#include <hip/hip_runtime.h>

#include "bootstrap.h"

namespace {

typedef unsigned long long u64;

// Philox4x32-10: the block of bootstrap.h (shared with gen.phiCI's draws), as the 16-byte pair of words a lane stores
__device__ __forceinline__ ulonglong2 philox_pair(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
    const genphi::PhiloxPair p = genphi::philox_pair(c0, c1, c2, c3, k0, k1);
    return make_ulonglong2(p.w0, p.w1);
}

// One meiosis over a pair of words: where T is set the parent's paternal copy a, else its maternal copy b
__device__ __forceinline__ ulonglong2 meiosis(ulonglong2 T, ulonglong2 a, ulonglong2 b)
{
    return make_ulonglong2((T.x & a.x) | (~T.x & b.x), (T.y & a.y) | (~T.y & b.y));
}

// the columns < S of the absolute word w
__device__ __forceinline__ u64 column_mask(long long S, long long w)
{
    const long long left = S - 64 * w;
    return left <= 0 ? 0ull : (left >= 64 ? ~0ull : (1ull << left) - 1);
}

}  // namespace
