// tree_keys.h -- the arithmetic of gen.phiTree (include/genphi.h: genphi_result_tree), written once for the device
// (tree.hip) and the host restatement (tree.cpp: genphi_tree_host): the edge test, the key of a row's best candidate, the key of a
// component's pick, and the order of the edges.  No HIP here: tree.cpp is a host-only unit.
//
// The order: edge (i, j), i < j, precedes (i', j') when its kinship is larger, then when i is smaller, then when j is smaller.
// Entries are finite and >= +0, so the unsigned bit pattern of a Float32 orders like its value.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GENPHI_TREE_HD __host__ __device__ inline
#else
#define GENPHI_TREE_HD inline
#endif

namespace genphi {

GENPHI_TREE_HD uint32_t tree_bits(float x)
{
    uint32_t b;
    __builtin_memcpy(&b, &x, sizeof b);
    return b;
}

GENPHI_TREE_HD float tree_value(uint32_t bits)
{
    float x;
    __builtin_memcpy(&x, &bits, sizeof x);
    return x;
}

// the edge test of gen.phiOver (over_device.h: over_at_least), one entry at a time
GENPHI_TREE_HD bool tree_is_edge(float x, double floor) { return static_cast<double>(x) >= floor; }

// The best candidate of row i.  For a fixed row the order of the edges {i, j} reduces to (kinship larger, then j smaller): a column
// j < i gives the edge (j, i), whose first position j is smaller than that of any edge (i, j') with j' > i, and among the columns on
// one side of i the edge order is the order of j.  So the larger key is the better candidate; 0 is "no candidate" (~j != 0 for every
// position j < 2^31).
constexpr uint64_t kTreeNoKey = 0;
GENPHI_TREE_HD uint64_t tree_row_key(uint32_t bits, int32_t j) { return (static_cast<uint64_t>(bits) << 32) | static_cast<uint32_t>(~j); }
GENPHI_TREE_HD uint32_t tree_row_key_bits(uint64_t key) { return static_cast<uint32_t>(key >> 32); }
GENPHI_TREE_HD int32_t tree_row_key_col(uint64_t key) { return static_cast<int32_t>(~static_cast<uint32_t>(key)); }

// The pick of a component, step 1: the largest kinship of its rows' candidates, kept as bits + 1 so that 0 is "no candidate" (a
// kinship of +0 is an edge when the floor is <= 0; the bits of a finite Float32 are below 2^32 - 1).
constexpr uint32_t kTreeNoLevel = 0;
GENPHI_TREE_HD uint32_t tree_level(uint64_t row_key) { return tree_row_key_bits(row_key) + 1u; }
GENPHI_TREE_HD uint32_t tree_level_bits(uint32_t level) { return level - 1u; }

// ... step 2: among the candidates at that kinship the smallest (min(i, j), max(i, j)); all ones is "none yet"
constexpr uint64_t kTreeNoPair = ~0ull;
GENPHI_TREE_HD uint64_t tree_pair_key(int32_t i, int32_t j)
{
    const uint32_t lo = static_cast<uint32_t>(i < j ? i : j), hi = static_cast<uint32_t>(i < j ? j : i);
    return (static_cast<uint64_t>(lo) << 32) | hi;
}
GENPHI_TREE_HD int32_t tree_pair_row(uint64_t pair) { return static_cast<int32_t>(pair >> 32); }
GENPHI_TREE_HD int32_t tree_pair_col(uint64_t pair) { return static_cast<int32_t>(pair & 0xFFFFFFFFu); }

// Two components that pick the same edge are one edge: it is emitted by the component of the smaller root.  `mine` and `theirs` are
// the roots of the picking component and of the one at the other end, `their_pair` the other one's pick.
GENPHI_TREE_HD bool tree_emits(int32_t mine, int32_t theirs, uint64_t my_pair, uint64_t their_pair) { return my_pair != their_pair || mine < theirs; }

// the order of the output list
GENPHI_TREE_HD bool tree_edge_before(uint32_t bits_a, uint64_t pair_a, uint32_t bits_b, uint64_t pair_b)
{
    return bits_a != bits_b ? bits_a > bits_b : pair_a < pair_b;
}

// the host stops after 40 rounds (never reached: a round that emits an edge at least halves the components that still grow)
constexpr int32_t kTreeMaxRounds = 40;

}  // namespace genphi
