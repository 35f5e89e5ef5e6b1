// carry.h -- the host side of gen.simuCarriers (the carriers of every founder allele among listed cases, by gene dropping; the
// definition is the text in include/genphi.h, genphi_carry_*).  The plan is gen.simuIdentity's (ident.h: plan_ident / IdentPlan) on the
// cases followed by the controls, unchanged.  Here: the two lists as sets of rows, the limits, what the sweep needs on the device and
// how the allele table is cut into label chunks, as pure functions.  No HIP: tests/carry_check.cpp builds it with g++.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "ident.h"

namespace genphi {

// The count kernel's workgroup: 16 waves; a wave's 64 lanes are the 64 simulations of a word.
constexpr int CARRY_THREADS = 1024;
// A counter dword holds c1 in bits 0-15, c2 in bits 16-30 and x in bit 31: with at most 32,767 distinct cases no field carries into the
// next (c2 <= c1 <= n < 2^15).
constexpr int64_t CARRY_MAX_CASES = 32767;
// The cells of carriers / homozygotes are addressed as l * W + c in an Int32 table of at most 2^31 - 1 entries.
constexpr int64_t CARRY_MAX_CELLS = 2147483647;
constexpr size_t CARRY_LDS_BYTES = 163840;
// The widest chunk: 64 tables of LC dwords, stride LC | 1 dwords apart, in 163,840 bytes of LDS: 256 (LC | 1) <= 163,840 gives
// LC | 1 <= 640, and the largest multiple of 32 with that is 608 (155,904 bytes).
constexpr int64_t CARRY_MAX_CHUNK = 608;
// The default chunk.  Reasoned first as 256 labels (65,792 bytes of LDS, two workgroups per CU); measured, the widest
// chunk was the fastest on all three bench inputs: every chunk decodes every listed side again, so the kernel's time follows the
// number of chunks (14,798 labels, 140 cases: 0.34 ms at 256, 0.24 ms at 608; 18,998 labels, 10,000 cases: 28.3 ms against 15.3 ms),
// and one workgroup per CU is no loss where the grid has thousands of them.
constexpr int64_t CARRY_DEFAULT_CHUNK = CARRY_MAX_CHUNK;

// The two lists as sets: the distinct rows of the cases, ascending, then the distinct rows of the controls, ascending.
struct CarryLists {
    std::vector<int32_t> rows;               // n_cases + n_controls rows of the panel
    int64_t n_cases = 0, n_controls = 0;
};

// pl.pro_row holds the rows of the listed cases (the first n_case_ids entries) and of the listed controls (the rest).  Returns true
// when an individual stands in both lists (GENPHI_ERR_ARG with the caller's text; its ID in both_id).
inline bool carry_lists(CarryLists &out, const IdentPlan &pl, int64_t n_case_ids, int64_t &both_id)
{
    out = CarryLists();
    std::vector<uint8_t> mark(static_cast<size_t>(pl.n_live), 0);
    const int64_t n_ids = static_cast<int64_t>(pl.pro_row.size());
    for (int64_t k = 0; k < n_ids; ++k) {
        const int32_t r = pl.pro_row[k];
        const uint8_t m = k < n_case_ids ? 1 : 2;
        if (mark[r] && mark[r] != m) {
            both_id = pl.row_id[r];
            return true;
        }
        mark[r] = m;
    }
    for (int64_t r = 0; r < pl.n_live; ++r)
        if (mark[r] == 1) out.rows.push_back(static_cast<int32_t>(r));
    out.n_cases = static_cast<int64_t>(out.rows.size());
    for (int64_t r = 0; r < pl.n_live; ++r)
        if (mark[r] == 2) out.rows.push_back(static_cast<int32_t>(r));
    out.n_controls = static_cast<int64_t>(out.rows.size()) - out.n_cases;
    return false;
}

// W: the columns of carriers / homozygotes for n distinct cases; max_count = 0: all of them.
inline int64_t carry_columns(int64_t n_cases, int64_t max_count) { return (max_count > 0 ? std::min(n_cases, max_count) : n_cases) + 1; }

// The limits of the definition; an empty string when they hold.
inline std::string carry_limits(int64_t n_cases, int64_t n_labels, int64_t W)
{
    if (n_cases < 1) return "no cases";
    if (n_cases > CARRY_MAX_CASES) return std::to_string(n_cases) + " distinct cases; at most 32,767 are counted";
    if (n_labels > CARRY_MAX_CELLS / W)
        return std::to_string(n_labels) + " founder alleles x " + std::to_string(W) + " columns are more than 2^31 - 1 cells; pass a smaller maxCount";
    return std::string();
}

// Device bytes of a sweep (carry.hip allocates exactly these; the check before any launch adds them up).
struct CarrySizes {
    size_t excluded = 0;         // Int32 n_labels
    size_t carriers = 0;         // Int32 n_labels x W
    size_t homozygotes = 0;      // Int32 n_labels x W
    size_t lists = 0;            // the parent rows, the IDs, the constant sides, the listed rows and the two sets of rows
    size_t pair_rows = 0;        // one pair of words of every live row: 2 sides x B planes x 16 bytes (ident_sizes')
    size_t fixed() const { return excluded + carriers + homozygotes + lists; }
    size_t panel(int64_t pairs) const { return pair_rows * static_cast<size_t>(pairs); }
};

inline CarrySizes carry_sizes(const IdentPlan &pl, const CarryLists &ls, int64_t W)
{
    CarrySizes z;
    z.excluded = 4 * static_cast<size_t>(pl.n_labels);
    z.carriers = z.homozygotes = 4 * static_cast<size_t>(pl.n_labels) * static_cast<size_t>(W);
    z.lists = label_list_bytes(pl) + 4 * ls.rows.size();
    z.pair_rows = 2 * 16 * static_cast<size_t>(pl.planes) * static_cast<size_t>(pl.n_live);
    return z;
}

// How the labels [0, n_labels) are cut into chunks of chunk_labels = LC: chunk c owns [c LC, min(n_labels, (c + 1) LC)).  A workgroup
// holds 64 tables (one per simulation of its word) of LC counter dwords, stride = LC | 1 dwords apart: lane s addresses dword
// s * stride + d, so for one d the 64 lanes fall on 64 different banks (an odd number is a unit modulo 32 and modulo 64).
struct CarryChunks {
    int64_t chunk_labels = 0;
    int64_t chunks = 0;
    int32_t stride = 0;
    size_t lds_bytes = 0;        // 64 * stride * 4
};

// chunk_arg: 0 = the default, CARRY_DEFAULT_CHUNK; a positive value is rounded up to a multiple of 32; either is then cut to
// CARRY_MAX_CHUNK and to n_labels.
inline CarryChunks carry_chunks(int64_t n_labels, int64_t chunk_arg)
{
    CarryChunks c;
    int64_t lc = chunk_arg > 0 ? (chunk_arg > CARRY_MAX_CHUNK ? CARRY_MAX_CHUNK : (chunk_arg + 31) / 32 * 32) : CARRY_DEFAULT_CHUNK;
    lc = std::max<int64_t>(1, std::min(lc, std::min(n_labels, CARRY_MAX_CHUNK)));
    c.chunk_labels = lc;
    c.chunks = n_labels > 0 ? (n_labels + lc - 1) / lc : 0;
    c.stride = static_cast<int32_t>(lc | 1);
    c.lds_bytes = 64 * 4 * static_cast<size_t>(c.stride);
    return c;
}

}  // namespace genphi
