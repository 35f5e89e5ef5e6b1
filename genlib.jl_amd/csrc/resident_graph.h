// resident_graph.h -- the host-side checks that the graph queries of the resident result share (clusters.hip: genphi_result_clusters,
// genphi_result_unrelated; tree.hip: genphi_result_tree): the full Float32 result, a piece of the plan's scratch block, and an error
// after launches were enqueued.  Every message goes out under the query's name.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <string>

#include "resident.h"

namespace genphi {

// These queries need the full Float32 result: not the Float64 one, not a row shard (an empty one too), a resident result.
inline int need_full_f32(const ResidentView &v, const char *name)
{
    if (v.res_f64) return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + " works on the Float32 result (gen.phi's matrix)");
    const bool empty = v.res_known && v.n_rows == 0;
    if (!empty && (!v.on_device || !v.result || v.n_rows == 0))
        return genphi_set_error(GENPHI_ERR_DEVICE, "no resident result: call genphi_compute_device first");
    if (empty || v.row_begin != 0 || v.n_rows != v.n_pro)
        return genphi_set_error(GENPHI_ERR_ARG, std::string(name) + ": " + std::to_string(v.n_rows) + " of " + std::to_string(v.n_pro) +
                                                    " rows are resident: the graph needs every row");
    if (v.ld < v.n_pro || v.ld % 64 != 0 || v.n_pro > INT32_MAX)
        return genphi_set_error(GENPHI_ERR_DEVICE, std::string(name) + ": unexpected row pitch " + std::to_string(v.ld));
    return GENPHI_OK;
}

inline int scratch_for(genphi_plan *p, size_t bytes, const char *name, const char *what, char **scratch)
{
    if (resident_scratch(p, bytes, scratch) == GENPHI_OK) return GENPHI_OK;
    return genphi_set_error(GENPHI_ERR_ALLOC, std::string(name) + ": " + std::to_string(bytes) + " bytes of device memory for " + what + ": " + genphi_last_error());
}

// after an error: the stream is drained (host arrays outlive what was enqueued), the error goes out under the query's name
inline int device_error(const ResidentView &v, hipError_t e, const char *name)
{
    (void)hipStreamSynchronize(v.stream);
    return genphi_set_error(GENPHI_ERR_DEVICE, std::string(name) + ": " + hipGetErrorString(e));
}

}  // namespace genphi
