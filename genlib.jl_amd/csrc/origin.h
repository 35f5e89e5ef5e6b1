// origin.h -- the host side of gen.simuOrigins (which founder alleles the kinship and the inbreeding of groups of probands descend from,
// by gene dropping; the definition is the text in include/genphi.h, genphi_origin_*).  The plan is gen.simuIdentity's (ident.h:
// plan_ident / IdentPlan) on the list as given, unchanged.  Here: the list as a set with its groups, the limits, what the sweep needs
// on the device and how the allele table is cut into label chunks, as pure functions.  No HIP: tests/origin_check.cpp builds it with g++.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

#include "ident.h"

namespace genphi {

// The count kernel's workgroup: 16 waves; a wave's 64 lanes are the 64 simulations of a word.
constexpr int ORIGIN_THREADS = 1024;
constexpr int32_t ORIGIN_MAX_GROUPS = 32;
// A counter dword holds c1 in bits 0-15 and c2 in bits 16-30: with at most 32,767 distinct probands in a group no field carries into
// the next (c2 <= c1 <= n_a < 2^15), and k = c1 + c2 <= 65,534 keeps a simulation's k_a k_b below 2^32.
constexpr int64_t ORIGIN_MAX_GROUP_SIZE = 32767;
// autozygous_pro is addressed as i * n_labels + l in an Int32 table of at most 2^31 - 1 entries.
constexpr int64_t ORIGIN_MAX_CELLS = 2147483647;
constexpr size_t ORIGIN_LDS_BYTES = 163840;

// Pair (a, b), a <= b < G, of the upper triangle, row-major: rows 0 .. a - 1 hold G, G - 1, .. entries.
inline int64_t origin_pair(int64_t a, int64_t b, int64_t G) { return a * G - a * (a - 1) / 2 + (b - a); }
inline int64_t origin_pairs(int64_t G) { return G * (G + 1) / 2; }

// The list as a set: the distinct probands with a group >= 0, sorted by group and then by row (the count kernel's row list), each with
// its group and its position among the distinct grouped probands in order of first appearance (the row of autozygous_pro).
struct OriginLists {
    std::vector<int32_t> rows, group, index;     // n entries each
    std::vector<int64_t> sizes;                  // n_a, G entries
    int64_t n = 0;
};

enum { ORIGIN_LIST_OK = 0, ORIGIN_LIST_RANGE = 1, ORIGIN_LIST_CONFLICT = 2 };

// pl.pro_row holds the rows of the listed entries; group: per entry -1 .. G - 1, or NULL (everyone in group 0).  ORIGIN_LIST_RANGE: the
// group of entry `bad` is outside -1 .. G - 1; ORIGIN_LIST_CONFLICT: the individual with the ID `bad` is listed with two different
// groups (-1 is a group of its own here).
inline int origin_lists(OriginLists &out, const IdentPlan &pl, const int32_t *group, int32_t G, int64_t &bad)
{
    out = OriginLists();
    out.sizes.assign(static_cast<size_t>(G), 0);
    std::vector<int32_t> of(static_cast<size_t>(pl.n_live), -2);         // -2: not listed so far
    std::vector<int32_t> first;                                           // the grouped rows by first appearance
    const int64_t n_ids = static_cast<int64_t>(pl.pro_row.size());
    for (int64_t k = 0; k < n_ids; ++k) {
        const int32_t r = pl.pro_row[k], g = group ? group[k] : 0;
        if (g < -1 || g >= G) {
            bad = k;
            return ORIGIN_LIST_RANGE;
        }
        if (of[r] == -2) {
            of[r] = g;
            if (g >= 0) first.push_back(r);
        } else if (of[r] != g) {
            bad = pl.row_id[r];
            return ORIGIN_LIST_CONFLICT;
        }
    }
    out.n = static_cast<int64_t>(first.size());
    std::vector<int32_t> perm(first.size());
    std::iota(perm.begin(), perm.end(), 0);
    std::sort(perm.begin(), perm.end(), [&](int32_t x, int32_t y) {
        const int32_t gx = of[first[x]], gy = of[first[y]];
        return gx != gy ? gx < gy : first[x] < first[y];
    });
    for (int32_t i : perm) {
        out.rows.push_back(first[i]);
        out.group.push_back(of[first[i]]);
        out.index.push_back(i);
        ++out.sizes[of[first[i]]];
    }
    return ORIGIN_LIST_OK;
}

// The limits of the definition; an empty string when they hold.
inline std::string origin_limits(const OriginLists &ls, int64_t n_labels, bool by_proband)
{
    if (ls.n < 1) return "no listed proband is in a group";
    for (size_t a = 0; a < ls.sizes.size(); ++a)
        if (ls.sizes[a] > ORIGIN_MAX_GROUP_SIZE)
            return std::to_string(ls.sizes[a]) + " distinct probands in group " + std::to_string(a) + "; at most 32,767 are counted";
    if (by_proband && n_labels > ORIGIN_MAX_CELLS / ls.n)
        return std::to_string(ls.n) + " probands x " + std::to_string(n_labels) + " founder alleles are more than 2^31 - 1 cells; ask without byProband";
    return std::string();
}

// Device bytes of a sweep (origin.hip allocates exactly these; the check before any launch adds them up).
struct OriginSizes {
    size_t copies = 0;           // Int64 G x n_labels
    size_t autozygous = 0;       // Int64 G x n_labels
    size_t matches = 0;          // Int64 G (G + 1) / 2 x n_labels
    size_t by_proband = 0;       // Int32 n x n_labels, when requested
    size_t lists = 0;            // the parent rows, the IDs, the constant sides, the listed rows and the row list with its groups and positions
    size_t pair_rows = 0;        // one pair of words of every live row: 2 sides x B planes x 16 bytes (ident_sizes')
    size_t fixed() const { return copies + autozygous + matches + by_proband + lists; }
    size_t panel(int64_t pairs) const { return pair_rows * static_cast<size_t>(pairs); }
};

inline OriginSizes origin_sizes(const IdentPlan &pl, const OriginLists &ls, int32_t G, bool by_proband)
{
    OriginSizes z;
    const size_t nl = static_cast<size_t>(pl.n_labels);
    z.copies = z.autozygous = 8 * static_cast<size_t>(G) * nl;
    z.matches = 8 * static_cast<size_t>(origin_pairs(G)) * nl;
    z.by_proband = by_proband ? 4 * static_cast<size_t>(ls.n) * nl : 0;
    z.lists = label_list_bytes(pl) + 4 * 3 * ls.rows.size();
    z.pair_rows = 2 * 16 * static_cast<size_t>(pl.planes) * static_cast<size_t>(pl.n_live);
    return z;
}

// How the labels [0, n_labels) are cut into chunks of chunk_labels = LC: chunk c owns [c LC, min(n_labels, (c + 1) LC)).  A workgroup
// holds 64 tables (one per simulation of its word) of LC x G counter dwords, the dword of (label t, group a) at t G + a, the tables
// stride = (LC G) | 1 dwords apart: lane s addresses dword s * stride + d, so for one d the 64 lanes fall on 64 different banks (an odd
// number is a unit modulo 32 and modulo 64).
struct OriginChunks {
    int64_t chunk_labels = 0;
    int64_t chunks = 0;
    int32_t stride = 0;
    size_t lds_bytes = 0;        // 64 * stride * 4
};

// The widest chunk of G groups: the largest LC with 256 ((LC G) | 1) <= 163,840, that is LC G <= 639: 639 labels at G = 1, 91 at
// G = 7, 19 at G = 32.
inline int64_t origin_max_chunk(int32_t G) { return (static_cast<int64_t>(ORIGIN_LDS_BYTES / 256) - 1) / G; }

// The default chunk, reasoned before anything was measured: the widest.  Every chunk decodes both sides of every listed proband again,
// so the count phase costs n x B x chunks whatever the width, and gen.simuCarriers' kernel, which decodes the same sides, was measured
// fastest at its widest chunk on every input (carry.h).  Against it stands one workgroup per CU (nothing hides the zeroing and the
// reduce of 160 KB of tables).  Measured against half the width, two workgroups per CU: half was slower on five of six
// (input, G) pairs (10,000 probands: 22.8 against 16.0 ms at G = 1, 155.9 against 106.0 ms at G = 7) and faster on one (14,798 labels,
// 140 probands, G = 1: 0.377 against 0.413 ms), so the widest stays.
inline int64_t origin_default_chunk(int32_t G) { return origin_max_chunk(G); }

// chunk_arg: 0 = the default; a positive value is taken as it is; either is then cut to origin_max_chunk(G) and to n_labels.
inline OriginChunks origin_chunks(int64_t n_labels, int32_t G, int64_t chunk_arg)
{
    OriginChunks c;
    int64_t lc = chunk_arg > 0 ? chunk_arg : origin_default_chunk(G);
    lc = std::max<int64_t>(1, std::min(lc, std::min(n_labels, origin_max_chunk(G))));
    c.chunk_labels = lc;
    c.chunks = n_labels > 0 ? (n_labels + lc - 1) / lc : 0;
    c.stride = static_cast<int32_t>((lc * G) | 1);
    c.lds_bytes = 64 * 4 * static_cast<size_t>(c.stride);
    return c;
}

}  // namespace genphi
