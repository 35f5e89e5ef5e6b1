// bootstrap.h -- the random draws of gen.phiCI / gen.fCI (include/genphi.h, genphi_bootstrap_counts and genphi_result_bootstrap)
// and the Philox4x32-10 block they share with gene dropping (simu.hip), written once for the host and the device so that the two
// cannot drift apart; and the interface between the entry point in result_queries.hip and the kernels in bootstrap.hip.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GENPHI_HD __host__ __device__ __forceinline__
#else
#define GENPHI_HD inline
#endif

namespace genphi {

struct PhiloxPair {
    uint64_t w0, w1;      // o0 | o1 << 32, o2 | o3 << 32
};

GENPHI_HD uint32_t mulhi_u32(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return static_cast<uint32_t>((static_cast<uint64_t>(a) * b) >> 32);
#endif
}

GENPHI_HD uint64_t mulhi_u64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * b) >> 64);
#endif
}

// Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0, k1); the pair of 64-bit words o0 | o1 << 32, o2 | o3 << 32
GENPHI_HD PhiloxPair philox_pair(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = mulhi_u32(M0, c0), lo0 = M0 * c0, hi1 = mulhi_u32(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    return PhiloxPair{static_cast<uint64_t>(c0) | (static_cast<uint64_t>(c1) << 32), static_cast<uint64_t>(c2) | (static_cast<uint64_t>(c3) << 32)};
}

// The two draws 2 * pair and 2 * pair + 1 of resample r among n probands (the second is not a draw when 2 * pair + 1 == n):
// one block with counter (pair, r, 0, 2); draw k takes word k & 1; the position is the high half of word * n.
struct BootDraws {
    int64_t s0, s1;
};
GENPHI_HD BootDraws boot_draws(uint64_t n, uint64_t seed, uint32_t r, uint32_t pair)
{
    const PhiloxPair w = philox_pair(pair, r, 0u, 2u, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
    return BootDraws{static_cast<int64_t>(mulhi_u64(w.w0, n)), static_cast<int64_t>(mulhi_u64(w.w1, n))};
}

#if defined(__HIPCC__)
// bootstrap.hip: quad[r] and self[r] of the resamples first .. first + n_boot - 1 over the resident rows, panel after panel on
// `stream`, then one copy of each to the host and a synchronise.  `scratch` holds boot_scratch_bytes(...) bytes.  Returns the
// first HIP error (no further panel is launched after one).
struct BootLaunch {
    hipStream_t stream;
    const float *phi;          // n_rows x ld, row k = proband row_begin + k; ld a multiple of 64, padding columns zero
    long long ld;
    int n, row_begin, n_rows;
    uint64_t seed;
    int first, n_boot;
    int panel;                 // resamples per panel (boot_panel)
    char *scratch;
    double *quad, *self;       // host, n_boot each; either may be NULL
};
int boot_panel(int n, int n_boot, int hook);                       // resamples per panel: the hook's value if >= 1, else the default rule
size_t boot_scratch_bytes(int n, int n_rows, int n_boot, int panel);
hipError_t boot_launch(const BootLaunch &L);
#endif

}  // namespace genphi
