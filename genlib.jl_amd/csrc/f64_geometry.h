// f64_geometry.h -- launch geometry of the Float64-storage level kernels of sweep_f64.hip (host only; no HIP here, so that
// tests/f64_geometry_check.cpp builds it with g++ and holds it to its invariants without a GPU).
//
// The kernels include it for the per-thread constants their register arrays are sized by; launch_level64 (sweep_f64.hip) asks
// f64_geometry for the numbers of a launch.  The two belong together: level_full64_kernel packs two source indices into 16 bits each and
// stages at most 2 * block * kF64Pre doubles of a row, so a block too small for the row is a silent wrong answer, not a crash.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace genphi {

constexpr int kF64Cols = 20;      // level_full64_kernel, columns per thread: ceil(10 304 / 512)  (ld of the widest cut whose rows fit)
constexpr int kF64Pre = 10;       // ... d2_t pieces per source row and thread: ceil(10 240 / 2 / 512)
constexpr int kS64Cols = 14;      // level_split64_kernel, columns per thread and chunk (registers: 7 per column + the 80 of the row in flight: 246 VGPRs, no scratch; 16 spills).
                                  // 14 instead of round 3's 12: genea140's widest cuts (13.7k columns) take 2 chunks instead of 3, i.e. a third fewer stagings
constexpr int kS64Pre = 20;       // ... d2_t pieces per source row and thread: 20,480 / 2 / 512

constexpr size_t kF64LdsMax = 160 * 1024;

// LDS a workgroup may fill with staged Float64 source rows: 160 KB, or the GENPHI_LDS_CAP_FLOATS test budget (4 bytes a
// float), which sends small cuts through level_split64_kernel / level_naive64_kernel too
inline size_t f64_lds_budget(int lds_cap_floats)
{
    return lds_cap_floats >= 16 ? std::min<size_t>(kF64LdsMax, 4 * static_cast<size_t>(lds_cap_floats)) : kF64LdsMax;
}

enum F64Form { kF64Full, kF64Split, kF64Naive };

struct F64Geometry {
    F64Form form;
    int block;                 // threads of a workgroup
    int grid_x, grid_y;        // full / split: persistent workgroups x column chunks; naive: rows x blocks of 256 columns
    int lds_row;               // doubles of a staged source row: n_prev + 1 in whole d2_t
    size_t lds_bytes;          // dynamic LDS: both source rows (full), one (split), none (naive)
};

// One level step from a cut of n_prev members to a matrix of row pitch ld, rows_n of its rows; kernel: opts.kernel (1 = per-entry only)
inline F64Geometry f64_geometry(int64_t n_prev, int64_t ld, int rows_n, int n_cus, int kernel, size_t lds_budget)
{
    F64Geometry g;
    g.lds_row = static_cast<int>((n_prev + 1 + 1) / 2 * 2);
    const size_t lds2 = 2 * static_cast<size_t>(g.lds_row) * sizeof(double), lds1 = static_cast<size_t>(g.lds_row) * sizeof(double);
    if (kernel != 1 && lds2 <= lds_budget && rows_n > 0) {
        // both Float64 source rows fit in LDS (cuts up to 10,239 members): the row-staged kernel
        g.form = kF64Full;
        // (columns per thread <= kF64Cols, row pieces per thread <= kF64Pre for each of these block sizes)
        const int bs = ld <= 64 * kF64Cols && g.lds_row <= 2 * 64 * kF64Pre ? 64 : (ld <= 256 * kF64Cols && g.lds_row <= 2 * 256 * kF64Pre ? 256 : 512);
        const int chunks = static_cast<int>((ld + bs * kF64Cols - 1) / (bs * kF64Cols));
        // resident workgroups per CU: LDS, and the kernel's ~240 VGPRs (two waves per SIMD)
        const int per_cu = static_cast<int>(std::min<size_t>(512 / bs, std::max<size_t>(1, kF64LdsMax / std::max<size_t>(lds2, 1))));
        g.block = bs; g.grid_x = std::min(rows_n, std::max(1, n_cus * per_cu / chunks)); g.grid_y = chunks; g.lds_bytes = lds2;
    } else if (kernel != 1 && lds1 <= lds_budget && rows_n > 0 && n_prev < 65535) {
        // one Float64 source row fits (cuts up to 20,479 members): the one-row-at-a-time kernel
        g.form = kF64Split;
        const int chunks = static_cast<int>((ld + 512 * kS64Cols - 1) / (512 * kS64Cols));
        g.block = 512; g.grid_x = std::min(rows_n, std::max(1, n_cus / chunks) * 2);     // (two pieces per CU and chunk: the tail)
        g.grid_y = chunks; g.lds_bytes = lds1;
    } else {
        g.form = kF64Naive;
        g.block = 256; g.grid_x = rows_n; g.grid_y = static_cast<int>((ld + 255) / 256); g.lds_bytes = 0;
    }
    return g;
}

}  // namespace genphi
