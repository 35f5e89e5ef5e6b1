// result_eigen.h -- the Lanczos core of genphi_result_eigen (include/genphi.h): a pure host function over basis slots
// that it reaches through callbacks, and the symmetric tridiagonal solver it uses.  No HIP here or in result_eigen.cpp:
// tests/eigen_check.cpp links both with host callbacks, csrc/eigen.hip hands them the device ones.
#pragma once
#include <cstdint>
#include <functional>

namespace genphi {

constexpr int32_t kEigenMaxIter = 4096;                      // the cap of max_iter (the basis is sized by it)
constexpr double kEigenBreakdown = 0x1p-40;                  // beta <= this x max_i(|alpha_i| + beta_i): the Krylov space is invariant
constexpr int32_t kEigenWork = -1;                           // EigenOps::set's slot number of the working vector w

// The vectors of the iteration live with the callee: basis slots 0 .. steps (n entries each) and one working vector w.  Every
// callback returns 0, or an error code that lanczos_top hands on.  h, S, theta and out are host arrays.
struct EigenOps {
    std::function<int(int32_t j, const double *x)> set;                          // slot j (kEigenWork: w) = x, n entries
    std::function<int(int32_t j)> apply;                                         // w = Op v_j
    std::function<int(int32_t m, double *h)> project;                            // h[i] = v_i . w, i < m
    std::function<int(int32_t m, const double *h)> subtract;                     // w -= sum over i < m of h[i] v_i, ascending i
    std::function<int(double *ww)> norm2;                                        // *ww = w . w
    std::function<int(int32_t j, double scale)> store;                           // v_j = scale w
    std::function<int(int32_t m, int32_t k, const double *S)> combine;           // u_c = sum over i < m of S[i * k + c] v_i, c < k
    std::function<int(int32_t k, const double *theta, double *out)> residuals;   // out[c] = || Op u_c - theta[c] u_c ||_2
    std::function<int(int32_t k, double *vectors, int64_t ldv)> download;        // vectors[e * ldv + c] = u_c[e]
};

// The k algebraically largest eigenpairs of the operator behind ops.apply by Lanczos with full reorthogonalisation; the iteration is
// written out in include/genphi.h at genphi_result_eigen.  values (k), vectors (n x k, pitch ldv); residual (k), converged (k) and
// products may be NULL.  center: the start and the fresh vectors are centred (the callee centres inside apply).  Nothing is written
// to an output unless the return value is 0.  Arguments are not checked here (1 <= k <= n, k <= max_iter).
int lanczos_top(int64_t n, int32_t k, bool center, double tol, int32_t max_iter, uint64_t seed, const EigenOps &ops,
                double *values, double *vectors, int64_t ldv, double *residual, int32_t *converged, int32_t *products);

// Eigenvalues of the symmetric tridiagonal matrix with diagonal d[0 .. n - 1] and sub-diagonal e[0 .. n - 2] (e[n - 1] is work space)
// by implicit QL.  On return d holds the eigenvalues, unsorted.  z is rows x n, row-major, and takes every rotation on its columns:
// handed the identity (rows = n) it returns the eigenvectors as columns; handed the last row of the identity (rows = 1) it returns
// their last components, in O(n^2) for the whole call.  False when an eigenvalue took more than 120 sweeps (not seen on finite input).
bool tridiagonal_ql(int32_t n, double *d, double *e, double *z, int32_t rows);

// the start stream: the next value of a splitmix64 generator as a double in [-1, 1)
double eigen_draw(uint64_t *state);

}  // namespace genphi
