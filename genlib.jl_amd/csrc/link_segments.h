// link_segments.h -- host side of gen.simuSegments (the lengths of the IBD segments of gen.simuSharing; the definition is the text in
// include/genphi.h, genphi_seg_*): the limits of a request, the bin of a length, the cells of the table, the check of a request, the
// device bytes it needs, and the walk over the runs of one masked `any` word, written once for the host and the device (as link.h
// does for the crossover word).  seg_walk_word is the only place that knows how a run crosses a word: link_segment_kernel (link.hip)
// and genphi_seg_host (link.cpp) both call it.  No HIP here: tests/segments_check.cpp builds it with g++.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "link.h"

namespace genphi {

constexpr int32_t kSegMaxEdges = 257;        // n_bins <= 256
constexpr int32_t kSegMaxEdge = 4097;        // kLinkMaxLoci + 1: the bin [1, L + 1) holds every length
constexpr int32_t kSegMaxGroups = 32;
constexpr int32_t kSegMaxCells = 2048;       // G (G + 1) / 2 x (n_bins + 2) cells of 24 bytes: 48 KB of LDS beside the tile

// The column k of a length in hist[a][b][k]: 0 = below edges[0], 1 + b = the bin [edges[b], edges[b + 1]), n_edges = at or above the
// last edge.  It is the number of edges <= len.
GENPHI_HD int32_t seg_bin(const int32_t *edges, int32_t n_edges, int32_t len)
{
    int32_t lo = 0, hi = n_edges;            // edges[0 .. lo) <= len < edges[hi ..)
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (edges[mid] <= len) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The table on the device keeps the pairs of groups a <= b only, row after row of the upper triangle; genphi_seg_to_host mirrors.
GENPHI_HD int32_t seg_group_pair(int32_t a, int32_t b, int32_t G)
{
    const int32_t lo = a < b ? a : b, hi = a < b ? b : a;
    return lo * G - lo * (lo - 1) / 2 + (hi - lo);
}

inline int64_t seg_cells(int32_t n_edges, int32_t n_groups)
{
    const int64_t G = n_groups > 1 ? n_groups : 1;
    return G * (G + 1) / 2 * (static_cast<int64_t>(n_edges) + 1);      // n_bins + 2 = n_edges + 1 columns
}

// The check of genphi_seg_request (n_edges >= 1): "" or the text of the error, which names the offending value.
inline std::string seg_check_request(int32_t n_edges, const int32_t *edges, int32_t min_loci, int32_t n_groups, const int32_t *group, int64_t n_pro)
{
    if (n_edges < 2 || n_edges > kSegMaxEdges) return std::to_string(n_edges) + " edges: need 2 .. 257";
    if (!edges) return "edges is NULL";
    if (edges[0] < 1) return "edges[0] = " + std::to_string(edges[0]) + " is below 1";
    for (int32_t k = 1; k < n_edges; ++k)
        if (edges[k] <= edges[k - 1])
            return "edges[" + std::to_string(k) + "] = " + std::to_string(edges[k]) + " does not exceed edges[" + std::to_string(k - 1) + "] = " +
                   std::to_string(edges[k - 1]) + ": the edges must be strictly increasing";
    if (edges[n_edges - 1] > kSegMaxEdge) return "edges[" + std::to_string(n_edges - 1) + "] = " + std::to_string(edges[n_edges - 1]) + " is above 4097";
    if (min_loci < 1 || min_loci > kSegMaxEdge) return "min_loci = " + std::to_string(min_loci) + " is outside 1 .. 4097";
    if (n_groups < 0 || n_groups > kSegMaxGroups) return std::to_string(n_groups) + " groups: at most 32";
    const int64_t cells = seg_cells(n_edges, n_groups);
    if (cells > kSegMaxCells)
        return std::to_string(cells) + " cells (" + std::to_string(n_groups) + " groups, " + std::to_string(n_edges - 1) + " bins): at most 2048";
    if (n_groups > 0) {
        if (!group) return "group is NULL with " + std::to_string(n_groups) + " groups";
        for (int64_t i = 0; i < n_pro; ++i)
            if (group[i] < -1 || group[i] >= n_groups)
                return "group[" + std::to_string(i) + "] = " + std::to_string(group[i]) + " is outside -1 .. " + std::to_string(n_groups - 1);
    }
    return "";
}

// Device bytes of a request (link.hip allocates exactly these; prepare() adds them to link_sizes' fixed bytes before any launch).
struct SegSizes {
    size_t table = 0;            // Int64 cells x 3
    size_t pairs = 0;            // Int64 n_pro x n_pro x 3
    size_t edges = 0;            // Int32 n_edges
    size_t labels = 0;           // Int32 n_pro (zeros without groups)
    size_t fixed() const { return table + pairs + edges + labels; }
};

inline SegSizes seg_sizes(int64_t n_pro, int32_t n_edges, int32_t n_groups)
{
    SegSizes z;
    if (n_edges == 0) return z;
    const size_t n = static_cast<size_t>(n_pro);
    z.table = 24 * static_cast<size_t>(seg_cells(n_edges, n_groups));
    z.pairs = 24 * n * n;
    z.edges = 4 * static_cast<size_t>(n_edges);
    z.labels = 4 * n;
    return z;
}

// the dynamic LDS of link_segment_kernel: the tile of the pair kernel, the table, the edges
inline size_t seg_lds_bytes(int32_t planes, int32_t n_edges, int32_t n_groups)
{
    return 2048 * static_cast<size_t>(planes) + 24 * static_cast<size_t>(seg_cells(n_edges, n_groups)) + 4 * static_cast<size_t>(n_edges);
}

// What a pair carries along the words of one simulation.  Reset per simulation: nothing open, no zero bit seen yet.
struct SegState {
    int32_t open = 0;            // the length of the open run, 0 = none
    int32_t longest = 0;         // the longest run closed so far
    bool from0 = true;           // no locus so far was unshared: a run open now, or opening next, began at locus 0
};

// One masked `any` word of `valid` = min(64, L - 64 w) >= 1 loci (the bits at and above `valid` are zero); last: w = W - 1.
// emit(length, censored) for every run that closes in this word; a run that reaches the top valid bit of a word other than the
// last stays open.  A run is censored when it holds locus 0 or locus L - 1.
template <typename Emit>
GENPHI_HD void seg_walk_word(uint64_t word, int32_t valid, bool last, SegState &st, Emit &&emit)
{
    if (word == 0 && st.open == 0) {         // the common word: nothing shared, nothing open
        st.from0 = false;
        return;
    }
    const uint64_t full = valid == 64 ? ~0ull : (1ull << valid) - 1;
    if (word == full) {                      // the other common word: shared throughout
        st.open += valid;
        if (last) {
            emit(st.open, true);
            if (st.open > st.longest) st.longest = st.open;
            st.open = 0;
        }
        return;
    }
    uint64_t x = word;                       // word >> pos
    int32_t pos = 0;
    while (pos < valid) {
        if (x & 1) {                         // ~x != 0: the word is not full, and the shifts brought zeros in
            const int32_t n = __builtin_ctzll(~x);
            st.open += n;
            pos += n;
            x >>= n;
            const bool end = pos == valid;
            if (end && !last) break;         // open across the border
            emit(st.open, st.from0 || end);
            if (st.open > st.longest) st.longest = st.open;
            st.open = 0;
        } else {
            if (st.open) {                   // (pos = 0) the run of the previous word ended at its bit 63
                emit(st.open, st.from0);
                if (st.open > st.longest) st.longest = st.open;
                st.open = 0;
            }
            st.from0 = false;
            if (x == 0) break;
            const int32_t n = __builtin_ctzll(x);
            pos += n;
            x >>= n;
        }
    }
}

// One pair and one simulation on the host, by the walk above: the chromosome's `any` as W words (bits at and above L ignored).
// hist: (n_edges + 1) x 3 (segments, loci, censored) and pair: 3 (segments >= min_loci, their loci, the longest); both added to.
inline void seg_reduce_host(int32_t L, const uint64_t *any_words, int32_t n_edges, const int32_t *edges, int32_t min_loci, int64_t *hist, int64_t *pair)
{
    SegState st;
    int64_t over = 0, over_loci = 0;
    const int32_t W = (L + 63) / 64;
    for (int32_t w = 0; w < W; ++w) {
        const int32_t valid = L - 64 * w < 64 ? L - 64 * w : 64;
        const uint64_t mask = valid == 64 ? ~0ull : (1ull << valid) - 1;
        seg_walk_word(any_words[w] & mask, valid, w == W - 1, st, [&](int32_t len, bool censored) {
            if (hist) {
                int64_t *cell = hist + 3 * seg_bin(edges, n_edges, len);
                cell[0] += 1;
                cell[1] += len;
                cell[2] += censored;
            }
            if (len >= min_loci) {
                over += 1;
                over_loci += len;
            }
        });
    }
    if (pair) {
        pair[0] += over;
        pair[1] += over_loci;
        pair[2] += st.longest;
    }
}

}  // namespace genphi
