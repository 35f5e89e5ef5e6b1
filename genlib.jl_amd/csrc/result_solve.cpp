// result_solve.cpp -- conjugate gradients over a product callback (result_solve.h; the iteration is stated in include/genphi.h at
// genphi_result_solve and in DESIGN.md 19).  Host only, no HIP: genphi_result_solve (matmul.hip) hands it the device product,
// tests/solve_check.cpp a host one.
#include "result_solve.h"

#include <cmath>
#include <cstddef>
#include <vector>

namespace genphi {

namespace {

// column c of an n x k array with pitch ld: plain ascending Float64 sums, so the same call gives the same bits
double dot(const double *a, int64_t lda, const double *b, int64_t ldb, int64_t n)
{
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += a[i * lda] * b[i * ldb];
    return s;
}

}  // namespace

int cg_solve(int64_t n, int32_t k, const double *b, int64_t ldb, double ridge, double tol, int32_t max_iter,
             const CgProduct &product, double *z, int64_t ldz, double *residual, int32_t *iterations)
{
    const size_t nk = static_cast<size_t>(n) * static_cast<size_t>(k);
    // column-major work arrays: column c at [c * n, (c + 1) * n)
    std::vector<double> zz(nk, 0.0), r(nk), d(nk);
    std::vector<double> rr(k), bnorm(k);
    std::vector<int32_t> its(k, 0), active;
    for (int32_t c = 0; c < k; ++c) {
        double *rc = r.data() + static_cast<size_t>(c) * n, *dc = d.data() + static_cast<size_t>(c) * n;
        for (int64_t i = 0; i < n; ++i) rc[i] = dc[i] = b[i * ldb + c];
        rr[c] = dot(rc, 1, rc, 1, n);
        bnorm[c] = std::sqrt(rr[c]);
        // a zero column is solved by z = 0; so is one that meets the tolerance at once (tol >= 1); NaN compares false: it runs
        if (!(bnorm[c] == 0.0) && !(bnorm[c] <= tol * bnorm[c])) active.push_back(c);
    }
    std::vector<double> px, py;
    for (int32_t it = 0; it < max_iter && !active.empty(); ++it) {
        const int32_t ka = static_cast<int32_t>(active.size());
        px.resize(static_cast<size_t>(n) * ka);
        py.resize(static_cast<size_t>(n) * ka);
        for (int32_t a = 0; a < ka; ++a) {
            const double *dc = d.data() + static_cast<size_t>(active[a]) * n;
            for (int64_t i = 0; i < n; ++i) px[static_cast<size_t>(i) * ka + a] = dc[i];
        }
        const int rc_ = product(ka, px.data(), py.data());
        if (rc_) return rc_;
        std::vector<int32_t> still;
        for (int32_t a = 0; a < ka; ++a) {
            const int32_t c = active[a];
            double *zc = zz.data() + static_cast<size_t>(c) * n, *rc = r.data() + static_cast<size_t>(c) * n, *dc = d.data() + static_cast<size_t>(c) * n;
            double *q = py.data() + a;                               // q = (Phi + ridge I) d, pitch ka
            for (int64_t i = 0; i < n; ++i) q[i * ka] += ridge * dc[i];
            ++its[c];
            const double dAd = dot(dc, 1, q, ka, n);
            if (!(dAd > 0.0) || !std::isfinite(dAd)) continue;       // breakdown: the column keeps the z it has
            const double alpha = rr[c] / dAd;
            for (int64_t i = 0; i < n; ++i) { zc[i] += alpha * dc[i]; rc[i] -= alpha * q[i * ka]; }
            const double rr_new = dot(rc, 1, rc, 1, n);
            if (std::sqrt(rr_new) <= tol * bnorm[c]) continue;       // converged by the recurrence residual
            const double beta = rr_new / rr[c];
            for (int64_t i = 0; i < n; ++i) dc[i] = rc[i] + beta * dc[i];
            rr[c] = rr_new;
            still.push_back(c);
        }
        active.swap(still);
    }
    // the true residual: one more product, of the columns that are not zero
    std::vector<double> res(k, 0.0);
    std::vector<int32_t> cols;
    for (int32_t c = 0; c < k; ++c)
        if (!(bnorm[c] == 0.0)) cols.push_back(c);
    if (!cols.empty()) {
        const int32_t kc = static_cast<int32_t>(cols.size());
        px.resize(static_cast<size_t>(n) * kc);
        py.resize(static_cast<size_t>(n) * kc);
        for (int32_t a = 0; a < kc; ++a) {
            const double *zc = zz.data() + static_cast<size_t>(cols[a]) * n;
            for (int64_t i = 0; i < n; ++i) px[static_cast<size_t>(i) * kc + a] = zc[i];
        }
        const int rc_ = product(kc, px.data(), py.data());
        if (rc_) return rc_;
        for (int32_t a = 0; a < kc; ++a) {
            const int32_t c = cols[a];
            const double *zc = zz.data() + static_cast<size_t>(c) * n;
            double s = 0.0;
            for (int64_t i = 0; i < n; ++i) {
                const double e = b[i * ldb + c] - (py[static_cast<size_t>(i) * kc + a] + ridge * zc[i]);
                s += e * e;
            }
            res[c] = std::sqrt(s) / bnorm[c];
        }
    }
    for (int32_t c = 0; c < k; ++c) {
        const double *zc = zz.data() + static_cast<size_t>(c) * n;
        for (int64_t i = 0; i < n; ++i) z[i * ldz + c] = zc[i];
        if (residual) residual[c] = res[c];
        if (iterations) iterations[c] = its[c];
    }
    return 0;
}

}  // namespace genphi
