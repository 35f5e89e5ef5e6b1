// bootstrap.cpp -- genphi_bootstrap_counts (include/genphi.h): the bootstrap draws of gen.phiCI / gen.fCI on the host, from the
// same header as the device's counts kernel (bootstrap.h).  No HIP here.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "../../include/genphi.h"
#include "bootstrap.h"
#include "error.h"

extern "C" int genphi_bootstrap_counts(int64_t n, uint64_t seed, int32_t first, int32_t n_boot, int32_t *counts)
{
    if (n < 2 || n > std::numeric_limits<int32_t>::max())
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_bootstrap_counts: n = " + std::to_string(n) + " outside [2, 2^31)");
    if (n_boot < 1 || first < 0 || first > std::numeric_limits<int32_t>::max() - n_boot)
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_bootstrap_counts: resamples first = " + std::to_string(first) + ", n_boot = " + std::to_string(n_boot) +
                                                    " (need first >= 0, n_boot >= 1, first + n_boot < 2^31)");
    if (!counts) return genphi_set_error(GENPHI_ERR_ARG, "genphi_bootstrap_counts: counts is NULL");
    const uint32_t pairs = static_cast<uint32_t>((n + 1) >> 1);
    auto rows = [&](int32_t b0, int32_t b1) {
        for (int32_t b = b0; b < b1; ++b) {
            int32_t *row = counts + static_cast<int64_t>(b) * n;
            std::memset(row, 0, static_cast<size_t>(n) * sizeof(int32_t));
            const uint32_t r = static_cast<uint32_t>(first) + static_cast<uint32_t>(b);
            for (uint32_t pair = 0; pair < pairs; ++pair) {
                const genphi::BootDraws d = genphi::boot_draws(static_cast<uint64_t>(n), seed, r, pair);
                ++row[d.s0];
                if (2 * static_cast<int64_t>(pair) + 1 < n) ++row[d.s1];
            }
        }
    };
    // resamples are independent: split them over a few threads once there is enough to do
    const int64_t work = static_cast<int64_t>(n_boot) * n;
    int threads = 1;
    if (work >= (int64_t(1) << 22)) {
        const unsigned hw = std::thread::hardware_concurrency();
        threads = static_cast<int>(std::min<int64_t>({16, hw ? hw : 1, n_boot}));
    }
    if (threads <= 1) {
        rows(0, n_boot);
        return GENPHI_OK;
    }
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) {
        const int32_t b0 = static_cast<int32_t>(static_cast<int64_t>(n_boot) * t / threads), b1 = static_cast<int32_t>(static_cast<int64_t>(n_boot) * (t + 1) / threads);
        pool.emplace_back(rows, b0, b1);
    }
    for (auto &th : pool) th.join();
    return GENPHI_OK;
}
