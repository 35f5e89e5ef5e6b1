// unique.h -- the host side of gen.simuUniqueness (the genome uniqueness of every proband: how much of what it carries is carried by
// nobody else of the population, by gene dropping; the definition is the text in include/genphi.h, genphi_unique_*).  The plan is
// gen.simuIdentity's (ident.h: plan_ident / IdentPlan) on the probands followed by the others, unchanged.  Here: the two lists as sets
// of rows, the columns, the limits, what the sweep needs on the device and how the allele table is cut into label chunks, as pure
// functions.  No HIP: tests/unique_check.cpp builds it with g++.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "carry.h"
#include "ident.h"

namespace genphi {

// The count kernel's workgroup: 16 waves; a wave's 64 lanes are the 64 simulations of a word.
constexpr int UNIQUE_THREADS = CARRY_THREADS;
// A counter is 16 bits, two labels to a dword: label t of a chunk lives in half t & 1 of dword t >> 1.  A field holds c1 <= n_pop, so
// with at most 65,535 members of the population it never passes 0xFFFF: adding 1 to the low half cannot carry into the high half, and
// adding 1 << 16 to the high half cannot carry out of the dword.  One 32-bit LDS atomic add therefore serves either half.
constexpr int64_t UNIQUE_MAX_POP = 65535;
// The cells of alleles / autozygous are addressed as i * K + column in an Int32 table of at most 2^31 - 1 entries.
constexpr int64_t UNIQUE_MAX_CELLS = 2147483647;
constexpr size_t UNIQUE_LDS_BYTES = CARRY_LDS_BYTES;
// The widest chunk: 64 tables of LC / 2 dwords, stride (LC / 2) | 1 dwords apart, in 163,840 bytes of LDS: 256 ((LC / 2) | 1) <= 163,840
// gives (LC / 2) | 1 <= 640, and the largest multiple of 64 with that is 1,216 (155,904 bytes): twice CARRY_MAX_CHUNK.
constexpr int64_t UNIQUE_MAX_CHUNK = 2 * CARRY_MAX_CHUNK;
// The default chunk.  Every chunk decodes the population once and the probands once more, so the kernel's time follows the number of
// chunks.  Measured against 640, which is what an argument of 608 rounds up to: 14,798 labels, 140 probands: 0.26 ms at
// 1,216 and 0.38 ms at 640; 18,998 labels, 10,000 probands: 16.8 ms against 32.0 ms; 3,776 labels, 2,000 probands: 1.78 ms against
// 1.55 ms, the one input where the narrower chunk won (4 chunks x 79 words are 316 workgroups of one per CU on 256 CUs).
constexpr int64_t UNIQUE_DEFAULT_CHUNK = UNIQUE_MAX_CHUNK;

// The two lists as sets: the distinct rows of the probands, ascending, then the distinct rows of the others that are not probands,
// ascending.  Together they are the population.
struct UniqueLists {
    std::vector<int32_t> rows;               // n_pro + n_others rows of the panel
    int64_t n_pro = 0, n_others = 0;
    int64_t n_pop() const { return n_pro + n_others; }
};

// pl.pro_row holds the rows of the listed probands (the first n_pro_ids entries) and of the listed others (the rest).  An individual
// in both lists is a proband.
inline void unique_lists(UniqueLists &out, const IdentPlan &pl, int64_t n_pro_ids)
{
    out = UniqueLists();
    std::vector<uint8_t> mark(static_cast<size_t>(pl.n_live), 0);
    const int64_t n_ids = static_cast<int64_t>(pl.pro_row.size());
    for (int64_t k = 0; k < n_ids; ++k) {
        const int32_t r = pl.pro_row[k];
        if (k < n_pro_ids) mark[r] = 1;
        else if (!mark[r]) mark[r] = 2;
    }
    for (int64_t r = 0; r < pl.n_live; ++r)
        if (mark[r] == 1) out.rows.push_back(static_cast<int32_t>(r));
    out.n_pro = static_cast<int64_t>(out.rows.size());
    for (int64_t r = 0; r < pl.n_live; ++r)
        if (mark[r] == 2) out.rows.push_back(static_cast<int32_t>(r));
    out.n_others = static_cast<int64_t>(out.rows.size()) - out.n_pro;
}

// K: the columns of alleles / autozygous for a population of n_pop; max_share = 0: all of them.  Column min(m, K) - 1 holds share m.
inline int64_t unique_columns(int64_t n_pop, int64_t max_share) { return max_share > 0 ? std::min(n_pop, max_share) : n_pop; }

// The limits of the definition; an empty string when they hold.
inline std::string unique_limits(int64_t n_pro, int64_t n_pop, int64_t K)
{
    if (n_pro < 1) return "no probands";
    if (n_pop > UNIQUE_MAX_POP) return std::to_string(n_pop) + " distinct probands and others; at most 65,535 are counted";
    if (n_pro > UNIQUE_MAX_CELLS / K)
        return std::to_string(n_pro) + " probands x " + std::to_string(K) + " columns are more than 2^31 - 1 cells; pass a smaller maxShare";
    return std::string();
}

// Device bytes of a sweep (unique.hip allocates exactly these; the check before any launch adds them up).
struct UniqueSizes {
    size_t alleles = 0;          // Int32 n x K
    size_t autozygous = 0;       // Int32 n x K
    size_t lists = 0;            // the parent rows, the IDs, the constant sides, the listed rows and the rows of the population
    size_t pair_rows = 0;        // one pair of words of every live row: 2 sides x B planes x 16 bytes (ident_sizes')
    size_t fixed() const { return alleles + autozygous + lists; }
    size_t panel(int64_t pairs) const { return pair_rows * static_cast<size_t>(pairs); }
};

inline UniqueSizes unique_sizes(const IdentPlan &pl, const UniqueLists &ls, int64_t K)
{
    UniqueSizes z;
    z.alleles = z.autozygous = 4 * static_cast<size_t>(ls.n_pro) * static_cast<size_t>(K);
    z.lists = label_list_bytes(pl) + 4 * ls.rows.size();
    z.pair_rows = 2 * 16 * static_cast<size_t>(pl.planes) * static_cast<size_t>(pl.n_live);
    return z;
}

// How the labels [0, n_labels) are cut into chunks of chunk_labels = LC: chunk c owns [c LC, min(n_labels, (c + 1) LC)).  A workgroup
// holds 64 tables (one per simulation of its word) of ceil(LC / 2) counter dwords, stride = ceil(LC / 2) | 1 dwords apart: lane s
// addresses dword s * stride + d, so for one d the 64 lanes fall on 64 different banks (an odd number is a unit modulo 32 and modulo
// 64).  An odd LC (only a table narrower than a chunk has one) leaves the high half of the last dword unused.
struct UniqueChunks {
    int64_t chunk_labels = 0;
    int64_t chunks = 0;
    int32_t stride = 0;
    size_t lds_bytes = 0;        // 64 * stride * 4
};

// chunk_arg: 0 = the default, UNIQUE_DEFAULT_CHUNK; a positive value is rounded up to a multiple of 64 and cut to UNIQUE_MAX_CHUNK;
// either is then cut to n_labels.
inline UniqueChunks unique_chunks(int64_t n_labels, int64_t chunk_arg)
{
    UniqueChunks c;
    int64_t lc = chunk_arg > 0 ? (chunk_arg > UNIQUE_MAX_CHUNK ? UNIQUE_MAX_CHUNK : (chunk_arg + 63) / 64 * 64) : UNIQUE_DEFAULT_CHUNK;
    lc = std::max<int64_t>(1, std::min(lc, std::min(n_labels, UNIQUE_MAX_CHUNK)));
    c.chunk_labels = lc;
    c.chunks = n_labels > 0 ? (n_labels + lc - 1) / lc : 0;
    c.stride = static_cast<int32_t>(((lc + 1) / 2) | 1);
    c.lds_bytes = 64 * 4 * static_cast<size_t>(c.stride);
    return c;
}

}  // namespace genphi
