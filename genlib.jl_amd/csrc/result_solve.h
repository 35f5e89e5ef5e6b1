// result_solve.h -- the conjugate-gradient core of genphi_result_solve (include/genphi.h): a pure host function over a
// product it is handed as a callback.  No HIP here or in result_solve.cpp: tests/solve_check.cpp links it with a host product.
#pragma once
#include <cstdint>
#include <functional>

namespace genphi {

// y = Phi x for kk columns at once: x and y are n x kk, dense row-major.  Returns 0, or an error code that cg_solve hands on.
// Column c of y must depend on column c of x alone (genphi_result_matmul's column property): cg_solve packs the columns that
// still run, so a column meets different neighbours from one product to the next.
using CgProduct = std::function<int(int32_t kk, const double *x, double *y)>;

// Solves (Phi + ridge I) z = b for the k columns of b (n x k, pitch ldb) by conjugate gradients from z = 0; the iteration is
// written out in include/genphi.h at genphi_result_solve.  z: n x k, pitch ldz; residual (k) and iterations (k) may be NULL.
// Nothing is written to z, residual or iterations unless the return value is 0.  Arguments are not checked here.
int cg_solve(int64_t n, int32_t k, const double *b, int64_t ldb, double ridge, double tol, int32_t max_iter,
             const CgProduct &product, double *z, int64_t ldz, double *residual, int32_t *iterations);

}  // namespace genphi
