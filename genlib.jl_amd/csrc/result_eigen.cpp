// result_eigen.cpp -- Lanczos with full reorthogonalisation over basis slots behind callbacks, and the implicit-QL solver of its
// tridiagonal matrix (result_eigen.h; the iteration is stated in include/genphi.h at genphi_result_eigen and in DESIGN.md 21).
// Host only, no HIP: genphi_result_eigen (eigen.hip) hands it the device vectors, tests/eigen_check.cpp host ones.
#include "result_eigen.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>
#include <numeric>
#include <vector>

namespace genphi {

double eigen_draw(uint64_t *state)
{
    uint64_t z = (*state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return 2.0 * (static_cast<double>(z >> 11) * 0x1p-53) - 1.0;
}

bool tridiagonal_ql(int32_t n, double *d, double *e, double *z, int32_t rows)
{
    if (n < 1) return true;
    e[n - 1] = 0.0;
    for (int32_t l = 0; l < n; ++l) {
        int sweeps = 0;
        int32_t m;
        do {
            for (m = l; m < n - 1; ++m) {                            // a negligible sub-diagonal entry splits the matrix
                const double dd = std::fabs(d[m]) + std::fabs(d[m + 1]);
                if (std::fabs(e[m]) + dd == dd) break;
            }
            if (m == l) break;
            if (++sweeps > 120) return false;
            double g = (d[l + 1] - d[l]) / (2.0 * e[l]);             // the Wilkinson shift
            double r = std::hypot(g, 1.0);
            g = d[m] - d[l] + e[l] / (g + std::copysign(r, g));
            double s = 1.0, c = 1.0, p = 0.0;
            int32_t i;
            for (i = m - 1; i >= l; --i) {
                double f = s * e[i];
                const double b = c * e[i];
                e[i + 1] = r = std::hypot(f, g);
                if (r == 0.0) {                                      // recover from underflow
                    d[i + 1] -= p;
                    e[m] = 0.0;
                    break;
                }
                s = f / r;
                c = g / r;
                g = d[i + 1] - p;
                r = (d[i] - g) * s + 2.0 * c * b;
                p = s * r;
                d[i + 1] = g + p;
                g = c * r - b;
                for (int32_t k = 0; k < rows; ++k) {                 // the rotation, on columns i and i + 1 of every row carried
                    double *zk = z + static_cast<size_t>(k) * n;
                    f = zk[i + 1];
                    zk[i + 1] = s * zk[i] + c * f;
                    zk[i] = c * zk[i] - s * f;
                }
            }
            if (r == 0.0 && i >= l) continue;
            d[l] -= p;
            e[l] = g;
            e[m] = 0.0;
        } while (m != l);
    }
    return true;
}

namespace {

// the next n draws of the stream, centred if asked (a plain ascending sum), then normalised; false when nothing is left to normalise
bool fresh_vector(int64_t n, bool center, uint64_t *state, std::vector<double> &x)
{
    for (int64_t e = 0; e < n; ++e) x[e] = eigen_draw(state);
    if (center) {
        double s = 0.0;
        for (int64_t e = 0; e < n; ++e) s += x[e];
        const double mean = s / static_cast<double>(n);
        for (int64_t e = 0; e < n; ++e) x[e] -= mean;
    }
    double ss = 0.0;
    for (int64_t e = 0; e < n; ++e) ss += x[e] * x[e];
    const double norm = std::sqrt(ss);
    if (!(norm > 0.0)) return false;
    for (int64_t e = 0; e < n; ++e) x[e] /= norm;
    return true;
}

// the positions of the entries of d, largest first (equal values by smaller position)
std::vector<int32_t> descending(const std::vector<double> &d)
{
    std::vector<int32_t> idx(d.size());
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&d](int32_t a, int32_t b) { return d[a] > d[b]; });
    return idx;
}

#define EIGEN_TRY(expr)            \
    do {                           \
        const int rc_ = (expr);    \
        if (rc_) return rc_;       \
    } while (0)

// w loses its components along v_0 .. v_(m - 1), twice (classical Gram-Schmidt); h1 and h2 keep the two sets of coefficients
int orthogonalise(const EigenOps &ops, int32_t m, std::vector<double> &h1, std::vector<double> &h2)
{
    EIGEN_TRY(ops.project(m, h1.data()));
    EIGEN_TRY(ops.subtract(m, h1.data()));
    EIGEN_TRY(ops.project(m, h2.data()));
    EIGEN_TRY(ops.subtract(m, h2.data()));
    return 0;
}

}  // namespace

int lanczos_top(int64_t n, int32_t k, bool center, double tol, int32_t max_iter, uint64_t seed, const EigenOps &ops,
                double *values, double *vectors, int64_t ldv, double *residual, int32_t *converged, int32_t *products)
{
    const int32_t steps = static_cast<int32_t>(std::min<int64_t>(max_iter, n));
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> alpha, beta;                                 // T: alpha[i] on the diagonal, beta[i] between i and i + 1
    std::vector<double> h1(static_cast<size_t>(steps) + 1), h2(static_cast<size_t>(steps) + 1), x(static_cast<size_t>(n));
    std::vector<double> d, e, last;
    std::vector<int32_t> flags(k, 0);                                // by rank, of the last convergence test
    uint64_t state = seed;
    bool finite = true;
    double scale = 0.0;                                              // max over the steps of |alpha_i| + beta_i

    if (fresh_vector(n, center, &state, x)) {
        EIGEN_TRY(ops.set(0, x.data()));
    } else {
        finite = false;                                              // (n = 1 and centred: the operator is zero, its start vector too)
    }
    int32_t m = 0;
    while (finite && m < steps) {
        EIGEN_TRY(ops.apply(m));
        ++m;                                                         // step m: the basis has m vectors, w = Op v_m
        EIGEN_TRY(orthogonalise(ops, m, h1, h2));
        double ww;
        EIGEN_TRY(ops.norm2(&ww));
        const double a = h1[m - 1] + h2[m - 1], b = std::sqrt(ww);
        if (!std::isfinite(a) || !std::isfinite(b)) {
            finite = false;
            break;
        }
        alpha.push_back(a);
        scale = std::max(scale, std::fabs(a) + b);
        if (b <= kEigenBreakdown * scale) {                          // the Krylov space is invariant
            beta.push_back(0.0);
            if (m >= k) {
                std::fill(flags.begin(), flags.end(), 1);
                break;
            }
            if (m == steps) break;
            if (!fresh_vector(n, center, &state, x)) break;
            EIGEN_TRY(ops.set(kEigenWork, x.data()));
            EIGEN_TRY(orthogonalise(ops, m, h1, h2));
            EIGEN_TRY(ops.norm2(&ww));
            const double left = std::sqrt(ww);
            if (!std::isfinite(left)) {
                finite = false;
                break;
            }
            if (left <= kEigenBreakdown) break;                      // nothing is left of a unit vector: the basis spans the space
            EIGEN_TRY(ops.store(m, 1.0 / left));
            continue;
        }
        beta.push_back(b);
        EIGEN_TRY(ops.store(m, 1.0 / b));
        if (m < k) continue;
        // Ritz values and the last components of T_m's eigenvectors: implicit QL carrying one row
        d.assign(alpha.begin(), alpha.end());
        e.assign(beta.begin(), beta.end());
        last.assign(m, 0.0);
        last[m - 1] = 1.0;
        if (!tridiagonal_ql(m, d.data(), e.data(), last.data(), 1)) {
            finite = false;
            break;
        }
        const std::vector<int32_t> idx = descending(d);
        const double bound = tol * d[idx[0]];
        bool all = true;
        for (int32_t c = 0; c < k; ++c) {
            flags[c] = b * std::fabs(last[idx[c]]) <= bound;
            all = all && flags[c];
        }
        if (all) break;
    }

    std::vector<double> val(k, nan), res(k, nan), vec(static_cast<size_t>(n) * k, nan);
    if (!finite) {
        std::fill(flags.begin(), flags.end(), 0);
    } else {
        // the pairs: all eigenvectors of T_m, once.  (Fewer than k steps happen only when the fresh vectors ran out: then m pairs.)
        const int32_t kk = std::min(k, m);
        d.assign(alpha.begin(), alpha.end());
        e.assign(beta.begin(), beta.end());
        e.resize(m, 0.0);
        std::vector<double> z(static_cast<size_t>(m) * m, 0.0);
        for (int32_t i = 0; i < m; ++i) z[static_cast<size_t>(i) * m + i] = 1.0;
        if (!tridiagonal_ql(m, d.data(), e.data(), z.data(), m)) {
            std::fill(flags.begin(), flags.end(), 0);
        } else {
            const std::vector<int32_t> idx = descending(d);
            std::vector<double> S(static_cast<size_t>(m) * kk), theta(kk), out(kk), got(static_cast<size_t>(n) * kk);
            for (int32_t c = 0; c < kk; ++c) {
                theta[c] = d[idx[c]];
                for (int32_t i = 0; i < m; ++i) S[static_cast<size_t>(i) * kk + c] = z[static_cast<size_t>(i) * m + idx[c]];
            }
            EIGEN_TRY(ops.combine(m, kk, S.data()));
            EIGEN_TRY(ops.residuals(kk, theta.data(), out.data()));
            EIGEN_TRY(ops.download(kk, got.data(), kk));
            for (int32_t c = 0; c < kk; ++c) {
                // the sign: the component of largest magnitude, the first of them, is positive
                int64_t big = 0;
                for (int64_t r = 1; r < n; ++r)
                    if (std::fabs(got[r * kk + c]) > std::fabs(got[big * kk + c])) big = r;
                const double sign = got[big * kk + c] < 0.0 ? -1.0 : 1.0;
                for (int64_t r = 0; r < n; ++r) vec[static_cast<size_t>(r) * k + c] = sign * got[r * kk + c];
                val[c] = theta[c];
                res[c] = out[c];
            }
            for (int32_t c = kk; c < k; ++c) flags[c] = 0;
        }
    }
    for (int32_t c = 0; c < k; ++c) {
        values[c] = val[c];
        for (int64_t r = 0; r < n; ++r) vectors[r * ldv + c] = vec[static_cast<size_t>(r) * k + c];
        if (residual) residual[c] = res[c];
        if (converged) converged[c] = flags[c];
    }
    if (products) *products = m;
    return 0;
}

}  // namespace genphi
