// over_device.h -- the edge test that the threshold queries of the resident result share (result_queries.hip: genphi_result_over;
// clusters.hip: genphi_result_clusters, genphi_result_unrelated): which of the four columns of a 16-byte quad of row i are at or
// above the threshold, and which of them count.  Every kernel tests the same bits with the same expression, so what one lists the
// others join.
#pragma once
#include <hip/hip_runtime.h>

namespace genphi {

constexpr int kOverTile = 1024;         // columns of a tile: 256 threads x one quad

// bit e = (double) entry e of the quad >= t
__device__ __forceinline__ unsigned over_at_least(const float4 v, double t)
{
    return (static_cast<double>(v.x) >= t ? 1u : 0u) | (static_cast<double>(v.y) >= t ? 2u : 0u) |
           (static_cast<double>(v.z) >= t ? 4u : 0u) | (static_cast<double>(v.w) >= t ? 8u : 0u);
}

__device__ __forceinline__ unsigned over_hits(const float4 v, int jq, int i, int n, double t)
{
    // bit e = column jq + e is listed: right of the diagonal, left of the padding, at or above the threshold
    const int lo = min(max(i + 1 - jq, 0), 4), hi = min(max(n - jq, 0), 4);
    const unsigned valid = (0xFu << lo) & ~(0xFu << hi) & 0xFu;
    const unsigned h = over_at_least(v, t);
    return h & valid;
}

// bit e = column jq + e is a neighbour of i: any column left of the padding but the diagonal, at or above the threshold
__device__ __forceinline__ unsigned over_row_hits(const float4 v, int jq, int i, int n, double t)
{
    const int hi = min(max(n - jq, 0), 4), d = i - jq;
    unsigned valid = ~(0xFu << hi) & 0xFu;
    if (d >= 0 && d < 4) valid &= ~(1u << d);
    return over_at_least(v, t) & valid;
}

}  // namespace genphi
