// group_tables.h -- the host tables of genphi_result_group_sums: pure index arithmetic, no HIP types, so that
// tests/host_sanitize.cpp can run it under the sanitizers.  The kernels that read the tables are in result_queries.hip.
#pragma once
#include <cstdint>
#include <vector>

namespace genphi {

constexpr int kGsMaxGroups = 4096;      // GENPHI_GROUP_SUMS_MAX_GROUPS
constexpr int kGsTile = 1024;           // columns of a tile: 256 threads x one quad
constexpr int kGsPiece = 16;
constexpr int kGsBlockRows = 64;
constexpr int kGsFan = 32;              // rows one thread of group_rows_reduce_kernel adds

struct GsPair { int x, y; };            // laid out as the device's int2

struct GroupTables {
    std::vector<int64_t> n_cols, n_rows;        // per group: labelled columns, resident rows
    int form = 0;                               // 0: every group's columns are one run; 1: labels in any order
    std::vector<int> rowlist;                   // resident rows sorted by group (stable)
    std::vector<GsPair> blocks;                 // (first entry of rowlist, rows): one group, at most kGsBlockRows rows
    // the rest is built only when there is a block
    int n_tiles = 0;
    std::vector<GsPair> tile_lists;             // (first A entry, first B entry); n_tiles + 1
    std::vector<int> list_a;                    // first column | columns << 16
    std::vector<GsPair> list_b;                 // (first piece | pieces << 16, group)
    std::vector<unsigned short> perm;           // form 1: each tile's labelled columns sorted by group
    int tiles_per_slab = 0, n_slabs = 0;
    int64_t n_part = 0;                         // blocks x slabs (the caller refuses more than INT32_MAX / 2)
    std::vector<std::vector<int>> level_beg;    // per level of the row reduction: first input row of every output row, + the end
    std::vector<int64_t> level_rows;            // ... and its output rows; the last level has one row per group
};

// group: N labels in [-1, n_groups), checked by the caller; the resident rows are [row_begin, row_begin + n_rows)
void build_group_tables(const int32_t *group, int n_groups, int64_t N, int64_t row_begin, int64_t n_rows, int n_cus, GroupTables &t);

}  // namespace genphi
