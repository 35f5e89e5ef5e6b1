// link.h -- host side of gen.simuSharing (linked-locus gene dropping; the definition is the text in include/genphi.h, genphi_link_*):
// the shape of a chromosome in words, the crossover word and its prefix written once for the host and the device (as bootstrap.h does
// for the Philox block, so that the two cannot drift apart), and what the sweep needs on the device as a pure function of the plan.
// The plan itself is gen.simuIdentity's (ident.h, plan_ident), unchanged.  No HIP here: tests/link_check.cpp builds it with g++.
#pragma once
#include <cstddef>
#include <cstdint>

#include "bootstrap.h"
#include "ident.h"

namespace genphi {

constexpr int32_t kLinkMaxLoci = 4096;       // W <= 64 words, Wp <= 32 pairs: a simulation never spans waves
constexpr int32_t kLinkMaxQ = 32768;         // r = q / 65536 <= 1/2

// A chromosome of L loci: W words of 64 loci, Wp pairs of words (a 16-byte element), and the lanes of the step kernel that own the
// pairs of one simulation: the power of two >= Wp.
struct LinkShape {
    int32_t L = 0, q = 0, W = 0, Wp = 0, lanes = 1;
};

inline LinkShape link_shape(int32_t L, int32_t q)
{
    LinkShape z;
    z.L = L;
    z.q = q;
    z.W = (L + 63) / 64;
    z.Wp = (z.W + 1) / 2;
    while (z.lanes < z.Wp) z.lanes *= 2;
    return z;
}

// The Philox blocks d = 0 .. 7 of a crossover word hold U_2d and U_2d+1.  The fold leaves acc = 0 until the lowest set bit of q, so
// the blocks below it are never drawn: the first block drawn, 8 when q = 0 (none).
GENPHI_HD int link_first_block(uint32_t q) { return q ? __builtin_ctz(q) >> 1 : 8; }

// Philox blocks of one (ID, side, simulation): those of its W crossover words and the one of the starting strand
inline int64_t link_blocks_per_side(const LinkShape &z) { return static_cast<int64_t>(z.W) * (8 - link_first_block(static_cast<uint32_t>(z.q))) + 1; }

// X(w) of (ID, side, simulation s): every bit set with probability q / 65536; in word 0, bit 0 is the strand the copy starts on.
GENPHI_HD uint64_t link_crossover_word(uint32_t id_lo, uint32_t id_hi, uint32_t s, uint32_t side, uint32_t w, uint32_t q, uint32_t k0, uint32_t k1)
{
    const uint32_t c3 = 0x80000000u | side | (w << 1);
    uint64_t acc = 0;
    for (int d = link_first_block(q); d < 8; ++d) {
        const PhiloxPair u = philox_pair(id_lo, id_hi, s, c3 | (static_cast<uint32_t>(d) << 8), k0, k1);
        acc = (q >> (2 * d)) & 1 ? acc | u.w0 : acc & u.w0;
        acc = (q >> (2 * d + 1)) & 1 ? acc | u.w1 : acc & u.w1;
    }
    if (w == 0) {
        const PhiloxPair u = philox_pair(id_lo, id_hi, s, c3 | (8u << 8), k0, k1);
        acc = (acc & ~1ull) | (u.w0 & 1ull);
    }
    return acc;
}

// the inclusive prefix XOR of the bits of a word, bit 0 first
GENPHI_HD uint64_t link_prefix_xor(uint64_t x)
{
    x ^= x << 1;
    x ^= x << 2;
    x ^= x << 4;
    x ^= x << 8;
    x ^= x << 16;
    x ^= x << 32;
    return x;
}

// link.cpp: X[0 .. W) and T[0 .. W) of (seed, ID, side, simulation s) for a chromosome of L loci at q; either may be NULL.  The host
// restatement of what the step kernel draws: the words one after the other, the parity carried from word to word.
void link_words(uint64_t seed, int64_t id, int32_t side, uint32_t s, const LinkShape &z, uint64_t *X, uint64_t *T);

// Device bytes of a sweep (link.hip allocates exactly these; the check before any launch adds them up).
struct LinkSizes {
    size_t sums = 0;             // Int64 n_pro x n_pro x 6
    size_t labels = 0;           // Int32 n_pro x 2 x S x L, under GENPHI_LINK_FLAG_LABELS
    size_t lists = 0;            // the parent rows, the IDs, the constant sides and the proband rows
    size_t sim_rows = 0;         // one simulation of every live row: Wp pairs of words x 2 sides x B planes x 16 bytes
    size_t sim_gather = 0;       // the same of the listed probands' rows (the pair kernel's dense copy)
    size_t fixed() const { return sums + labels + lists; }
    size_t panel(int64_t sims) const { return (sim_rows + sim_gather) * static_cast<size_t>(sims); }
};

inline LinkSizes link_sizes(const IdentPlan &pl, int64_t S, const LinkShape &shape, bool labels)
{
    LinkSizes z;
    const size_t n_pro = static_cast<size_t>(pl.n_pro), sim_side = 16 * static_cast<size_t>(pl.planes) * static_cast<size_t>(shape.Wp);
    z.sums = 48 * n_pro * n_pro;
    z.labels = labels ? 8 * n_pro * static_cast<size_t>(S) * static_cast<size_t>(shape.L) : 0;
    z.lists = label_list_bytes(pl);
    z.sim_rows = 2 * sim_side * static_cast<size_t>(pl.n_live);
    z.sim_gather = 2 * sim_side * n_pro;
    return z;
}

}  // namespace genphi
