// matmul_device.h -- genphi_result_matmul's launch for a caller whose panel is on the device already (matmul.hip defines both;
// eigen.hip is the caller).  The kernel, its forms and the bits of the product are those of genphi_result_matmul.
#pragma once
#include <hip/hip_runtime.h>

#include "resident.h"

namespace genphi {

// the columns of the device panel of a k-column product: k rounded up to the column tile of its kernel form (1, 2, 4, 8, 16 n)
int matmul_panel_columns(int k);

// Enqueues y = Phi x for the resident rows on v.stream.  d_x: the panel, column c at d_x + c * n4, n4 = N rounded up to 4; rows
// N .. n4 - 1 and the columns k .. matmul_panel_columns(k) - 1 must hold +0.  d_y: n_rows x k, dense row-major.  1 <= k <= 64.
hipError_t matmul_on_device(const ResidentView &v, int n4, int k, const double *d_x, double *d_y);

}  // namespace genphi
