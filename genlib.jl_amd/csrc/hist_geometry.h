// hist_geometry.h -- the host arithmetic of genphi_result_hist and genphi_result_select (csrc/hist.hip): which rows a workgroup
// walks, the Float32 form of the Float64 edges, and the bytes of the plan's scratch block.  Host only: no HIP include, so that
// tests/hist_geometry_check.cpp compiles it with g++ alone.  include/genphi.h states the contract, DESIGN.md 20 the design.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

namespace genphi {

constexpr int kHistThreads = 256;                        // threads of a workgroup: 4 waves
constexpr int kHistTile = 4 * kHistThreads;              // columns of a tile: one quad per thread
constexpr int kHistChunksPerCu = 8;                      // chunks (= workgroups) asked for per compute unit
constexpr int64_t kHistChunkPairLimit = int64_t(1) << 31;   // a chunk holds FEWER pairs than this: its Int32 LDS counters cannot wrap
constexpr int kSelectDigitBits = 8;                      // a radix pass of genphi_result_select takes this many bits of the pattern
constexpr int kSelectDigits = 1 << kSelectDigitBits;
constexpr int kSelectPasses = 32 / kSelectDigitBits;
static_assert(32 % kSelectDigitBits == 0, "the passes cover the 32 bits of an entry exactly");

// pairs (i, j), i < j < n, of row i
inline int64_t hist_row_pairs(int64_t n, int64_t i) { return n - 1 - i; }

// ... of the rows [r0, r1), 0 <= r0 <= r1 <= n: the closed form of the sum (n < 2^31, so every product is below 2^62)
inline int64_t hist_pairs_of_rows(int64_t n, int64_t r0, int64_t r1)
{
    const int64_t m = r1 - r0;
    return m * (n - 1) - (r0 + r1 - 1) * m / 2;          // (r0 + r1 - 1) m = 2 (r0 + ... + r1 - 1): even
}

// The walk of a call: `order` lists the resident rows that can hold a counted pair -- not row n - 1, not a row without a label
// when there are labels -- sorted by (label, row), and begin[c] .. begin[c + 1] are the positions of chunk c.  The chunks are
// contiguous, none is empty, and each holds fewer than `limit` pairs, a row weighing hist_row_pairs whatever its columns' labels.
struct HistChunks {
    std::vector<int32_t> order, begin;
    int64_t pairs = 0;                                   // of all rows of `order`
    int n_chunks() const { return begin.empty() ? 0 : static_cast<int>(begin.size()) - 1; }
};

// group: NULL, or n labels in [-1, n_groups).  want: the number of chunks asked for (>= 1); there are more only where the limit
// forces a cut, and never more than rows.
inline HistChunks hist_chunks(int64_t n, int64_t r0, int64_t r1, const int32_t *group, int n_groups, int64_t want,
                              int64_t limit = kHistChunkPairLimit)
{
    HistChunks h;
    r1 = std::min(r1, n - 1);                            // row n - 1 has no pair
    if (r1 <= r0) return h;
    if (!group) {
        h.order.resize(static_cast<size_t>(r1 - r0));
        for (int64_t i = r0; i < r1; ++i) h.order[static_cast<size_t>(i - r0)] = static_cast<int32_t>(i);
    } else {                                             // a counting sort by label keeps the rows of a label ascending
        std::vector<int64_t> at(static_cast<size_t>(n_groups) + 1, 0);
        for (int64_t i = r0; i < r1; ++i)
            if (group[i] >= 0) ++at[static_cast<size_t>(group[i]) + 1];
        for (int g = 0; g < n_groups; ++g) at[static_cast<size_t>(g) + 1] += at[static_cast<size_t>(g)];
        h.order.resize(static_cast<size_t>(at[static_cast<size_t>(n_groups)]));
        for (int64_t i = r0; i < r1; ++i)
            if (group[i] >= 0) h.order[static_cast<size_t>(at[static_cast<size_t>(group[i])]++)] = static_cast<int32_t>(i);
    }
    if (h.order.empty()) return h;
    for (const int32_t i : h.order) h.pairs += hist_row_pairs(n, i);
    const int64_t quota = std::max<int64_t>(1, (h.pairs + std::max<int64_t>(want, 1) - 1) / std::max<int64_t>(want, 1));
    int64_t cur = 0;
    h.begin.push_back(0);
    for (size_t pos = 0; pos < h.order.size(); ++pos) {
        const int64_t w = hist_row_pairs(n, h.order[pos]);          // (one row alone: w <= n - 1 < 2^31 <= limit for n < 2^31)
        if (pos > static_cast<size_t>(h.begin.back()) && (cur >= quota || cur + w >= limit)) {
            h.begin.push_back(static_cast<int32_t>(pos));
            cur = 0;
        }
        cur += w;
    }
    h.begin.push_back(static_cast<int32_t>(h.order.size()));
    return h;
}

// The edges as Float32 thresholds.  An entry x is a Float32, so for a Float64 edge e
//     (double)x >= e  <=>  x >= hist_float_at_or_above(e)      and      (double)x > e  <=>  x >= hist_float_above(e):
// between a Float32 and the next one there is no x to tell e from the upper one.  The kernel compares Float32 with Float32 and
// still decides every comparison as the Float64 definition does, for every double e, +-inf included.
inline float hist_float_at_or_above(double e)            // the smallest Float32 f with (double)f >= e (+inf when e > FLT_MAX)
{
    float f = static_cast<float>(e);                     // to nearest: one step below at worst
    if (static_cast<double>(f) < e) f = std::nextafter(f, std::numeric_limits<float>::infinity());
    return f;
}
inline float hist_float_above(double e)                  // the smallest Float32 f with (double)f > e; NaN (never <= x) for e = +inf
{
    float f = hist_float_at_or_above(e);
    if (static_cast<double>(f) == e) {
        if (std::isinf(f) && f > 0) return std::numeric_limits<float>::quiet_NaN();
        f = std::nextafter(f, std::numeric_limits<float>::infinity());
    }
    return f;
}

// t[0 .. n_edges): t[b] = at_or_above(edges[b]) for b < n_bins, t[n_bins] = above(edges[n_bins]).  With k = #{b : t[b] <= x}
// (the t ascend, a NaN comes last, so the b counted are a prefix): k = 0 is `below`, k = n_edges is `above`, else x is in bin
// k - 1 -- the last bin takes x == edges[n_bins], numpy's rule.  Two edges between the same two Float32 give equal thresholds:
// the bin between them is empty in Float64 too.
inline std::vector<float> hist_thresholds(int32_t n_edges, const double *edges)
{
    std::vector<float> t(static_cast<size_t>(n_edges));
    for (int32_t b = 0; b + 1 < n_edges; ++b) t[static_cast<size_t>(b)] = hist_float_at_or_above(edges[b]);
    t[static_cast<size_t>(n_edges) - 1] = hist_float_above(edges[n_edges - 1]);
    return t;
}
// the same count on the host (binary search is the kernel's; this is the definition)
inline int32_t hist_count_at_or_below(const std::vector<float> &t, float x)
{
    int32_t k = 0;
    while (k < static_cast<int32_t>(t.size()) && t[static_cast<size_t>(k)] <= x) ++k;
    return k;
}

// The first guess of k - 1 for uniform edges: (x - t[0]) * scale, to be verified against t (hist.hip).  0 where the outer edges
// give no finite positive width: the guess is then bin 0, and the verification sends every other entry to the search.
inline float hist_guess_scale(int32_t n_edges, const double *edges)
{
    const double width = edges[n_edges - 1] - edges[0];
    if (!(width > 0) || !std::isfinite(width)) return 0.0f;
    const double s = static_cast<double>(n_edges - 1) / width;
    return s < 1.0e30 ? static_cast<float>(s) : 0.0f;
}

// The plan's scratch block of one call, every part 256-byte aligned.  Cells are uint64.
//   hist:   cells = G G (n_edges + 1), G = max(n_groups, 1): [row label][column label][below, bins, above]
//   select: cells = kSelectDigits per live prefix, GENPHI_SELECT_MAX_RANKS prefixes at most
struct HistScratch {
    size_t order = 0, begin = 0, label = 0, thr = 0, table = 0, total = 0;       // byte offsets, and the size of the block
};
inline size_t hist_al256(size_t b) { return (b + 255) / 256 * 256; }
inline HistScratch hist_scratch(size_t n_order, size_t n_chunks, size_t n_label, size_t n_thr, size_t cells)
{
    HistScratch s;
    s.order = 0;
    s.begin = s.order + hist_al256(n_order * sizeof(int32_t));
    s.label = s.begin + hist_al256((n_chunks + 1) * sizeof(int32_t));
    s.thr = s.label + hist_al256(n_label * sizeof(int32_t));
    s.table = s.thr + hist_al256(n_thr * sizeof(float));
    s.total = s.table + hist_al256(cells * sizeof(uint64_t));
    return s;
}
inline size_t hist_cells(int32_t n_edges, int32_t n_groups)
{
    const size_t g = static_cast<size_t>(std::max(n_groups, 1));
    return g * g * (static_cast<size_t>(n_edges) + 1);
}
// labels on the device: one per column, padded with -1 to a whole quad
inline size_t hist_label_entries(int64_t n, bool grouped) { return grouped ? static_cast<size_t>((n + 3) / 4 * 4) : 0; }
// bytes of dynamic LDS of the hist kernel: the thresholds, then the table [column label][n_edges + 1] of Int32
inline size_t hist_lds_bytes(int32_t n_edges, int32_t n_groups)
{
    return (static_cast<size_t>(n_edges) + static_cast<size_t>(std::max(n_groups, 1)) * (static_cast<size_t>(n_edges) + 1)) * 4;
}

}  // namespace genphi
