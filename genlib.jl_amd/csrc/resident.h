// resident.h -- what a query of the finished resident result may see of a plan (result_queries.hip, result_to_host.cpp), and nothing
// else of it: genphi_hip.hip keeps genphi_plan private and defines the three accessors below.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/genphi.h"

int genphi_set_error(int code, const std::string &msg);      // genphi_hip.hip

namespace genphi {

// keys of the LDS buffer of nearest_kernel (GENPHI_NEAREST_BUF): powers of two, >= 2 x GENPHI_NEAREST_MAX_K
constexpr int kNearBufMin = 128, kNearBufMax = 4096, kNearBufDefault = 1024;
// the buffer a plan uses: the hook's value clamped to [kNearBufMin, kNearBufMax] and rounded down to a power of two
inline int nearest_buf_entries(int hook)
{
    if (hook <= 0) return kNearBufDefault;
    int b = kNearBufMin;
    while (b * 2 <= (hook < kNearBufMax ? hook : kNearBufMax)) b *= 2;
    return b;
}

// The hooks the queries read (README.md, "Environment hooks"); tuning_from in genphi_hip.hip fills them when the plan is created.
struct ResultTuning {
    int d2h_threads = 0;           // GENPHI_D2H_THREADS      tuning: worker threads of genphi_result_to_host
    bool d2h_pageable = false;     // GENPHI_D2H_PAGEABLE     A-B: no pinned staging ring
    int d2h_sym = -1;              // GENPHI_D2H_SYM          opt-in: 1 = a full result crosses the link as upper-triangle tiles + a host mirror pass (default: every entry is copied)
    int d2h_tile_rows = 0, d2h_tile_cols = 0;   // GENPHI_D2H_TILE "RxC"  test + tuning: tile of the symmetric copy (default 256 x 8192)
    int d2h_chunk_mb = 0;          // GENPHI_D2H_CHUNK_MB     tuning: size of a pinned staging chunk of genphi_result_to_host (default 16, 4 for results below 2 GB)
    int boot_panel = 0;            // GENPHI_BOOT_PANEL       tuning + test: resamples per panel of genphi_result_bootstrap, 1 .. 8192 (default: what keeps a panel's counts within 256 MiB)
    int nearest_buf = kNearBufDefault;   // GENPHI_NEAREST_BUF     tuning + test: keys of the LDS buffer of genphi_result_nearest, a power of two in [128, 4096] (default 1024; the result
                                   //                         does not depend on it: tests force 128 so that small inputs cut the buffer on every tile)
};

struct ResidentView {
    int device, n_cus;
    hipStream_t stream;
    int64_t n_pro;
    const float *result;           // n_rows x ld, row k = proband row_begin + k; ld a multiple of 64, padding columns zero
    const double *result64;        // ... of a Float64-storage sweep (res_f64)
    int64_t ld, row_begin, n_rows;
    bool on_device, res_f64;
    bool res_known;                // a genphi_compute_device call has set the resident row range (it may be empty)
    const ResultTuning *tun;
};
ResidentView resident_view(const genphi_plan *p);

// the plan's scratch block, grown to >= bytes (contents undefined): *scratch.  The error is set on failure.
int resident_scratch(genphi_plan *p, size_t bytes, char **scratch);

// genphi_result_over: offsets (exclusive scan of the per-row counts, n_rows + 1 entries) of the last threshold counted on the resident
// result, so that a count-only call followed by a filling call runs the counting pass once.  The plan drops it whenever the result is
// recomputed or released.
struct OverCache {
    std::vector<int64_t> off;
    double threshold = 0.0;
    bool valid = false;
    void drop() { valid = false; off.clear(); }
};
OverCache &resident_over_cache(genphi_plan *p);

inline size_t al256(size_t b) { return (b + 255) / 256 * 256; }

// Messages name a HIP call by `what`.  Where a call moved here from genphi_hip.hip, `what` is the text its message had there (the
// expression as it was spelled on the plan): frozen message text, not code -- it is not meant to follow later renames.
#define GENPHI_RESIDENT_TRY(what, expr)                                                                            \
    do {                                                                                                           \
        hipError_t e_ = (expr);                                                                                    \
        if (e_ != hipSuccess) return genphi_set_error(GENPHI_ERR_DEVICE, std::string(what ": ") + hipGetErrorString(e_)); \
    } while (0)

}  // namespace genphi
