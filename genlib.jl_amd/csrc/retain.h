// retain.h -- the host side of gen.simuRetention (founder allele survival by gene dropping; the definition is the text in
// include/genphi.h, genphi_retain_*).  The plan is gen.simuIdentity's (ident.h: plan_ident / IdentPlan), unchanged.  Here: what the
// sweep needs on the device and how the allele table is cut into label chunks, as pure functions.  No HIP: tests/retain_check.cpp
// builds it with g++.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "ident.h"

namespace genphi {

// Device bytes of a sweep (retain.hip allocates exactly these; the check before any launch adds them up).
struct RetainSizes {
    size_t survived = 0;         // Int32 n_labels
    size_t both = 0;             // Int32 n_labels
    size_t distinct = 0;         // Int32 S
    size_t lists = 0;            // the parent rows, the IDs, the constant sides and the proband rows
    size_t pair_rows = 0;        // one pair of words of every live row: 2 sides x B planes x 16 bytes (ident_sizes')
    size_t fixed() const { return survived + both + distinct + lists; }
    size_t panel(int64_t pairs) const { return pair_rows * static_cast<size_t>(pairs); }
};

inline RetainSizes retain_sizes(const IdentPlan &pl, int64_t S)
{
    RetainSizes z;
    z.survived = z.both = 4 * static_cast<size_t>(pl.n_labels);
    z.distinct = 4 * static_cast<size_t>(S);
    z.lists = label_list_bytes(pl);
    z.pair_rows = 2 * 16 * static_cast<size_t>(pl.planes) * static_cast<size_t>(pl.n_live);
    return z;
}

// The mark kernel's workgroup: 16 waves; a wave's 64 lanes are the 64 simulations of a word.
constexpr int RETAIN_THREADS = 1024;
// The widest chunk: 64 bitmaps of 16,384 bits are 128 KiB; with the halo bit and the odd stride 131,328 of the 163,840 bytes of LDS.
constexpr int64_t RETAIN_MAX_CHUNK = 16384;
// The default chunk.  Reasoned first as RETAIN_MAX_CHUNK (decode every side as few times as possible); measured, 8,192
// labels were faster or equal on all three bench inputs: 65,792 bytes of LDS let two workgroups share a CU, and a table of 14,798
// labels gives 160 workgroups instead of 80 on 256 CUs.
constexpr int64_t RETAIN_DEFAULT_CHUNK = 8192;

// How the labels [0, n_labels) are cut into chunks of chunk_labels = LC: chunk c owns [c LC, min(n_labels, (c + 1) LC)).  A
// workgroup holds 64 bitmaps (one per simulation of its word) of LC + 1 bits: bit LC is the halo, the first label of the next
// chunk.  bitmap_dwords = LC / 32 + 1 dwords hold them; stride = that made odd, in dwords, the distance between the bitmaps
// of neighbouring simulations: lane s addresses dword s * stride + d, so for one d the 64 lanes fall on 64 different banks
// (an odd number is a unit modulo 32 and modulo 64).
struct RetainChunks {
    int64_t chunk_labels = 0;
    int64_t chunks = 0;
    int32_t bitmap_dwords = 0;
    int32_t stride = 0;
    size_t lds_bytes = 0;        // 64 * stride * 4
};

// chunk_arg: 0 = the default, the whole table up to RETAIN_DEFAULT_CHUNK labels, else chunks of that many; a positive value is
// rounded up to a multiple of 32, then cut to n_labels and to RETAIN_MAX_CHUNK.  So the first label of every chunk is a multiple of
// 32: a dword of a bitmap holds 32 consecutive labels from a multiple of 32.
inline RetainChunks retain_chunks(int64_t n_labels, int64_t chunk_arg)
{
    RetainChunks c;
    int64_t lc = chunk_arg > 0 ? (chunk_arg > RETAIN_MAX_CHUNK ? RETAIN_MAX_CHUNK : (chunk_arg + 31) / 32 * 32) : RETAIN_DEFAULT_CHUNK;
    lc = std::max<int64_t>(1, std::min(lc, std::min(n_labels, RETAIN_MAX_CHUNK)));
    c.chunk_labels = lc;
    c.chunks = n_labels > 0 ? (n_labels + lc - 1) / lc : 0;
    c.bitmap_dwords = static_cast<int32_t>(lc / 32 + 1);
    c.stride = c.bitmap_dwords | 1;
    c.lds_bytes = 64 * 4 * static_cast<size_t>(c.stride);
    return c;
}

// The mark phase that ships (0: plain atomicOr; 1: read the word first and skip the atomic when the bit is set); either can be
// forced by a create flag (include/genphi.h).  DESIGN.md 25 records the measurement behind the choice.
constexpr int RETAIN_DEFAULT_TEST_FIRST = 0;

}  // namespace genphi
