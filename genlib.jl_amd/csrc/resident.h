// resident.h -- what a query of the finished resident result may see of a plan (result_queries.hip, result_to_host.cpp), and nothing
// else of it: genphi_plan (plan_device.h) stays with the sweep's two units, and genphi_hip.hip defines the three accessors below.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/genphi.h"
#include "tuning.h"      // ResultTuning, nearest_buf_entries
#include "error.h"

namespace genphi {

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
