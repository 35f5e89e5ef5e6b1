// eigen_check.cpp -- the Lanczos core of genphi_result_eigen (csrc/result_eigen.cpp: genphi::lanczos_top, genphi::tridiagonal_ql)
// without a GPU: a stand-alone program that hands it host callbacks over a dense Float64 matrix and checks what include/genphi.h
// promises of the iteration.  Built by tests/test_eigen_host.py with g++, once plain and once under AddressSanitizer +
// UndefinedBehaviorSanitizer.
//
// Matrices with a known spectrum: A = H D H, H = I - 2 v v^T / (v^T v) a Householder reflection, D = diag(lam).  The bounds, with
// u = 2^-53, m the steps taken and lam_1 the largest eigenvalue:
//   rounding           = 8 (n + m + 2) u lam_1: a product's (n + 2) u |A| |x| <= (n + 2) u sqrt(n)-free bound in the 2-norm is
//                        <= (n + 2) u ||A||_F; H D H itself is formed with n-term sums, and a Ritz vector is a sum of m terms.
//                        The factor 8 covers the two reorthogonalisation passes, the scaling and the construction of A.
//   |theta_i - lam_i|  <= residual_i + rounding for a converged pair whose eigenvalue is simple (Weyl / the residual bound: some
//                        eigenvalue lies within the residual; the cases keep the top k + 1 eigenvalues further apart than that)
//   residual_i         <= tol theta_1 + rounding where the pair is flagged converged
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../genlib.jl_amd/csrc/result_eigen.h"

namespace {

int violations = 0;
long matrices = 0, pairs = 0, products = 0;
const double U = std::ldexp(1.0, -53);

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            ++violations;                                  \
            std::fprintf(stderr, "VIOLATION %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);             \
            std::fprintf(stderr, "\n");                    \
        }                                                  \
    } while (0)

// host vectors behind genphi::EigenOps; fail_op / fail_at: the call of that op that returns 77
struct Host {
    int64_t n;
    bool centre;
    std::vector<double> a;                                  // n x n row-major
    std::vector<std::vector<double>> slot;
    std::vector<double> w, u;                               // u: k columns of n
    int fail_op = -1;
    long fail_at = 0, calls[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};

    int tick(int op) { return op == fail_op && calls[op]++ == fail_at ? 77 : 0; }
    std::vector<double> &vec(int32_t j)
    {
        if (j == genphi::kEigenWork) return w;
        if (static_cast<size_t>(j) >= slot.size()) slot.resize(j + 1);
        slot[j].resize(n);
        return slot[j];
    }
    void centre_vec(std::vector<double> &x) const
    {
        double s = 0.0;
        for (double e : x) s += e;
        for (double &e : x) e -= s / static_cast<double>(n);
    }
    std::vector<double> op(std::vector<double> x) const
    {
        if (centre) centre_vec(x);
        std::vector<double> y(n);
        for (int64_t i = 0; i < n; ++i) {
            double s = 0.0;
            for (int64_t j = 0; j < n; ++j) s += a[i * n + j] * x[j];
            y[i] = s;
        }
        if (centre) centre_vec(y);
        return y;
    }
    genphi::EigenOps ops()
    {
        genphi::EigenOps o;
        w.assign(n, 0.0);
        o.set = [this](int32_t j, const double *x) {
            if (int rc = tick(0)) return rc;
            vec(j).assign(x, x + n);
            return 0;
        };
        o.apply = [this](int32_t j) {
            if (int rc = tick(1)) return rc;
            ++products;
            w = op(vec(j));
            return 0;
        };
        o.project = [this](int32_t m, double *h) {
            if (int rc = tick(2)) return rc;
            for (int32_t i = 0; i < m; ++i) {
                double s = 0.0;
                for (int64_t e = 0; e < n; ++e) s += slot[i][e] * w[e];
                h[i] = s;
            }
            return 0;
        };
        o.subtract = [this](int32_t m, const double *h) {
            if (int rc = tick(3)) return rc;
            for (int32_t i = 0; i < m; ++i)
                for (int64_t e = 0; e < n; ++e) w[e] -= h[i] * slot[i][e];
            return 0;
        };
        o.norm2 = [this](double *ww) {
            if (int rc = tick(4)) return rc;
            double s = 0.0;
            for (double e : w) s += e * e;
            *ww = s;
            return 0;
        };
        o.store = [this](int32_t j, double scale) {
            if (int rc = tick(5)) return rc;
            std::vector<double> &v = vec(j);
            for (int64_t e = 0; e < n; ++e) v[e] = w[e] * scale;
            return 0;
        };
        o.combine = [this](int32_t m, int32_t k, const double *S) {
            if (int rc = tick(6)) return rc;
            u.assign(static_cast<size_t>(n) * k, 0.0);
            for (int32_t c = 0; c < k; ++c)
                for (int32_t i = 0; i < m; ++i)
                    for (int64_t e = 0; e < n; ++e) u[static_cast<size_t>(c) * n + e] += S[static_cast<size_t>(i) * k + c] * slot[i][e];
            return 0;
        };
        o.residuals = [this](int32_t k, const double *theta, double *out) {
            if (int rc = tick(7)) return rc;
            for (int32_t c = 0; c < k; ++c) {
                std::vector<double> x(u.begin() + static_cast<size_t>(c) * n, u.begin() + static_cast<size_t>(c + 1) * n);
                const std::vector<double> y = op(x);
                double s = 0.0;
                for (int64_t e = 0; e < n; ++e) s += (y[e] - theta[c] * x[e]) * (y[e] - theta[c] * x[e]);
                out[c] = std::sqrt(s);
            }
            return 0;
        };
        o.download = [this](int32_t k, double *vectors, int64_t ldv) {
            if (int rc = tick(8)) return rc;
            for (int64_t e = 0; e < n; ++e)
                for (int32_t c = 0; c < k; ++c) vectors[e * ldv + c] = u[static_cast<size_t>(c) * n + e];
            return 0;
        };
        return o;
    }
};

// A = H diag(lam) H with the Householder vector v
Host similar(const std::vector<double> &lam, const std::vector<double> &v, bool centre)
{
    const int64_t n = static_cast<int64_t>(lam.size());
    double vv = 0.0;
    for (double e : v) vv += e * e;
    std::vector<double> h(n * n);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < n; ++j) h[i * n + j] = (i == j ? 1.0 : 0.0) - 2.0 * v[i] * v[j] / vv;
    Host m{n, centre, std::vector<double>(n * n), {}, {}, {}};
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int64_t l = 0; l < n; ++l) s += h[i * n + l] * lam[l] * h[l * n + j];
            m.a[i * n + j] = m.a[j * n + i] = s;
        }
    ++matrices;
    return m;
}

Host similar(const std::vector<double> &lam, std::mt19937_64 &rng, bool centre = false)
{
    std::normal_distribution<double> nor;
    std::vector<double> v(lam.size());
    for (double &e : v) e = nor(rng);
    return similar(lam, v, centre);
}

// eigenvalues (descending) of a dense symmetric matrix by cyclic Jacobi
std::vector<double> jacobi(std::vector<double> a, int64_t n)
{
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int64_t i = 0; i < n; ++i)
            for (int64_t j = 0; j < i; ++j) off += a[i * n + j] * a[i * n + j];
        if (off == 0.0) break;
        for (int64_t p = 0; p < n; ++p)
            for (int64_t q = p + 1; q < n; ++q) {
                if (a[p * n + q] == 0.0) continue;
                const double theta = (a[q * n + q] - a[p * n + p]) / (2.0 * a[p * n + q]);
                const double t = std::copysign(1.0, theta) / (std::fabs(theta) + std::hypot(theta, 1.0));
                const double c = 1.0 / std::hypot(t, 1.0), s = t * c;
                for (int64_t r = 0; r < n; ++r) {
                    const double x = a[r * n + p], y = a[r * n + q];
                    a[r * n + p] = c * x - s * y;
                    a[r * n + q] = s * x + c * y;
                }
                for (int64_t r = 0; r < n; ++r) {
                    const double x = a[p * n + r], y = a[q * n + r];
                    a[p * n + r] = c * x - s * y;
                    a[q * n + r] = s * x + c * y;
                }
            }
    }
    std::vector<double> d(n);
    for (int64_t i = 0; i < n; ++i) d[i] = a[i * n + i];
    std::sort(d.begin(), d.end(), [](double x, double y) { return x > y; });
    return d;
}

constexpr double kSentinel = -7.0;

struct Out {
    int rc;
    std::vector<double> val, vec, res;                       // vec: n x k dense
    std::vector<int32_t> conv;
    int32_t prod;
};

// one call with a pitch beyond k; checks what holds for every finite case: descending values, unit vectors, the sign rule, mutual
// orthogonality, the reported residual against a recomputed one, untouched gaps
Out run(Host &m, int k, double tol, int max_iter, uint64_t seed, bool expect_finite = true)
{
    const int64_t n = m.n, ldv = k + 2;
    Out o{0, std::vector<double>(k, kSentinel), std::vector<double>(n * k), std::vector<double>(k, kSentinel), std::vector<int32_t>(k, -7), -7};
    std::vector<double> vectors(n * ldv, kSentinel);
    const genphi::EigenOps ops = m.ops();
    o.rc = genphi::lanczos_top(n, k, m.centre, tol, max_iter, seed, ops, o.val.data(), vectors.data(), ldv, o.res.data(), o.conv.data(), &o.prod);
    for (int64_t r = 0; r < n; ++r) {
        for (int c = 0; c < k; ++c) o.vec[r * k + c] = vectors[r * ldv + c];
        CHECK(vectors[r * ldv + k] == kSentinel && vectors[r * ldv + k + 1] == kSentinel, "a gap of vectors was written");
    }
    if (o.rc != 0 || !expect_finite) return o;
    pairs += k;
    CHECK(o.prod >= 1 && o.prod <= std::min<int64_t>(max_iter, n), "products = %d", o.prod);
    double top = 0.0;
    for (int64_t i = 0; i < n * n; ++i) top = std::max(top, std::fabs(m.a[i]));
    const double rounding = 8.0 * (n + o.prod + 2) * U * top * n;        // (||A||_2 <= n max|a|)
    for (int c = 0; c < k; ++c) {
        if (std::isnan(o.val[c])) continue;                              // (pairs that a run of fresh vectors could not supply)
        if (c) CHECK(o.val[c - 1] >= o.val[c], "values not descending at %d", c);
        double ss = 0.0, big = 0.0;
        int64_t at = 0;
        std::vector<double> x(n);
        for (int64_t r = 0; r < n; ++r) {
            x[r] = o.vec[r * k + c];
            ss += x[r] * x[r];
            if (std::fabs(x[r]) > big) { big = std::fabs(x[r]); at = r; }
        }
        CHECK(std::fabs(ss - 1.0) <= 64.0 * (n + o.prod) * U, "n = %ld pair %d: |v|^2 - 1 = %g", (long)n, c, ss - 1.0);
        CHECK(x[at] > 0.0, "n = %ld pair %d: the largest component is negative", (long)n, c);
        for (int c2 = 0; c2 < c; ++c2) {
            double dot = 0.0;
            for (int64_t r = 0; r < n; ++r) dot += x[r] * o.vec[r * k + c2];
            CHECK(std::fabs(dot) <= 64.0 * (n + o.prod) * U, "n = %ld pairs %d, %d: v.v = %g", (long)n, c2, c, dot);
        }
        const std::vector<double> y = m.op(x);
        double rr = 0.0;
        for (int64_t r = 0; r < n; ++r) rr += (y[r] - o.val[c] * x[r]) * (y[r] - o.val[c] * x[r]);
        CHECK(std::fabs(std::sqrt(rr) - o.res[c]) <= rounding, "n = %ld pair %d: residual %g, recomputed %g", (long)n, c, o.res[c], std::sqrt(rr));
        if (o.conv[c]) CHECK(o.res[c] <= tol * o.val[0] + rounding, "n = %ld pair %d: converged with residual %g > %g", (long)n, c, o.res[c], tol * o.val[0] + rounding);
        CHECK(o.conv[c] == 0 || o.conv[c] == 1, "flag %d", o.conv[c]);
    }
    return o;
}

void known_spectra(std::mt19937_64 &rng)
{
    for (int64_t n : {1, 2, 3, 4, 5, 8, 17, 33, 64, 100, 200}) {
        std::vector<double> lam(n);
        for (int64_t i = 0; i < n; ++i) lam[i] = 1.0 / static_cast<double>(1 + i);      // simple, the top ones well apart
        Host m = similar(lam, rng);
        for (int k : {1, 3, 10}) {
            if (k > n) continue;
            const double tol = 1e-10;
            Out o = run(m, k, tol, 300, 1 + k);
            CHECK(o.rc == 0, "rc = %d", o.rc);
            for (int c = 0; c < k; ++c) {
                CHECK(o.conv[c] == 1, "n = %ld k = %d pair %d did not converge in %d steps", (long)n, k, c, o.prod);
                CHECK(std::fabs(o.val[c] - lam[c]) <= o.res[c] + 8.0 * (2 * n + 2) * U * n, "n = %ld k = %d value %d: %.17g for %.17g (residual %g)", (long)n, k, c,
                      o.val[c], lam[c], o.res[c]);
            }
        }
    }
    // k = N: the whole spectrum; the iteration ends in a breakdown at step N
    for (int64_t n : {1, 2, 3, 7, 20}) {
        std::vector<double> lam(n);
        for (int64_t i = 0; i < n; ++i) lam[i] = 2.0 - 0.09 * static_cast<double>(i);
        Host m = similar(lam, rng);
        Out o = run(m, static_cast<int>(n), 1e-10, 300, 5);
        CHECK(o.rc == 0 && o.prod == n, "k = N = %ld: rc %d, %d products", (long)n, o.rc, o.prod);
        for (int c = 0; c < n; ++c)
            CHECK(o.conv[c] == 1 && std::fabs(o.val[c] - lam[c]) <= o.res[c] + 64.0 * n * n * U * 2.0, "k = N = %ld value %d: %.17g for %.17g", (long)n, c, o.val[c], lam[c]);
    }
}

void multiple_and_invariant(std::mt19937_64 &rng)
{
    {   // a triple top eigenvalue is reported once; the list goes on with the next distinct ones
        std::vector<double> lam(200);
        // (the next two lie close to the top and far above the rest: they converge before rounding noise along the other two
        // directions of the triple eigenvalue, of the order u at every step, has been amplified into a copy -- include/genphi.h)
        for (int i = 0; i < 200; ++i) lam[i] = i < 3 ? 1.0 : i == 3 ? 0.9 : i == 4 ? 0.8 : 0.1 - 0.0005 * (i - 5);
        Host m = similar(lam, rng);
        Out o = run(m, 3, 1e-8, 300, 9);
        CHECK(o.prod < 60, "multiple top: %d products", o.prod);
        const double want[3] = {1.0, lam[3], lam[4]};
        for (int c = 0; c < 3; ++c) CHECK(o.rc == 0 && o.conv[c] == 1 && std::fabs(o.val[c] - want[c]) <= o.res[c] + 1e-12, "multiple top: value %d = %.17g, want %.17g", c, o.val[c], want[c]);
    }
    for (int64_t n : {1, 7, 70}) {   // I / 2: a breakdown at every step, fresh vectors until k
        const int k = static_cast<int>(std::min<int64_t>(n, 5));
        Host m{n, false, std::vector<double>(n * n, 0.0), {}, {}, {}};
        for (int64_t i = 0; i < n; ++i) m.a[i * n + i] = 0.5;
        ++matrices;
        Out o = run(m, k, 1e-8, 300, 3);
        CHECK(o.rc == 0 && o.prod == k, "I / 2, n = %ld: rc %d, %d products for k = %d", (long)n, o.rc, o.prod, k);
        for (int c = 0; c < k; ++c) CHECK(o.val[c] == 0.5 && o.conv[c] == 1 && o.res[c] <= 16 * U, "I / 2, n = %ld: pair %d = %.17g, residual %g", (long)n, c, o.val[c], o.res[c]);
    }
    for (int k : {1, 2, 3}) {   // A = 2 q q^T + 0.3 (I - q q^T): the start vector spans a 2-dimensional invariant subspace with q
        const int64_t n = 12;
        std::vector<double> q(n), lam(n, 0.3);
        std::normal_distribution<double> nor;
        for (double &e : q) e = nor(rng);
        lam[0] = 2.0;
        // H with Householder vector q - |q| e_0 maps e_0 to q / |q|: then A = H diag(2, .3, ..) H
        double qq = 0.0;
        for (double e : q) qq += e * e;
        std::vector<double> v = q;
        v[0] -= std::sqrt(qq);
        Host m = similar(lam, v, false);
        Out o = run(m, k, 1e-10, 300, 11);
        CHECK(o.rc == 0 && o.prod == std::max(k, 2), "invariant subspace, k = %d: rc %d, %d products", k, o.rc, o.prod);
        for (int c = 0; c < k; ++c) CHECK(o.conv[c] == 1 && std::fabs(o.val[c] - (c ? 0.3 : 2.0)) <= 1e-13, "invariant subspace, k = %d: value %d = %.17g", k, c, o.val[c]);
    }
    {   // the start vector itself an eigenvector: a breakdown at step 1
        const int64_t n = 9;
        uint64_t state = 21;
        std::vector<double> x(n), lam(n, 0.3);
        for (double &e : x) e = genphi::eigen_draw(&state);
        lam[0] = 2.0;
        double xx = 0.0;
        for (double e : x) xx += e * e;
        std::vector<double> v = x;
        v[0] -= std::sqrt(xx);
        Host m = similar(lam, v, false);
        Out o = run(m, 2, 1e-10, 300, 21);
        CHECK(o.rc == 0 && o.prod == 2 && std::fabs(o.val[0] - 2.0) <= 1e-13 && std::fabs(o.val[1] - 0.3) <= 1e-13 && o.conv[0] == 1 && o.conv[1] == 1,
              "start eigenvector: rc %d, %d products, values %.17g %.17g", o.rc, o.prod, o.val[0], o.val[1]);
    }
}

void limits_and_centring(std::mt19937_64 &rng)
{
    std::vector<double> lam(100);
    for (int i = 0; i < 100; ++i) lam[i] = 1.0 / (1 + i);
    Host m = similar(lam, rng);
    Out o = run(m, 5, 1e-10, 5, 2);                             // max_iter = k: it returns, the flags agree with the residuals (run)
    CHECK(o.rc == 0 && o.prod == 5, "max_iter = k: rc %d, %d products", o.rc, o.prod);
    std::vector<double> l20(lam.begin(), lam.begin() + 20);
    Host m20 = similar(l20, rng);
    o = run(m20, 3, 0.0, 300, 2);                               // tol = 0: to the breakdown at step N
    CHECK(o.rc == 0 && o.prod == 20, "tol = 0: rc %d, %d products", o.rc, o.prod);
    for (int c = 0; c < 3; ++c) CHECK(o.conv[c] == 1 && std::fabs(o.val[c] - l20[c]) <= 1e-13, "tol = 0: value %d = %.17g", c, o.val[c]);
    // the same call twice: the same bytes
    Out o2 = run(m20, 3, 0.0, 300, 2);
    CHECK(o.val == o2.val && o.vec == o2.vec && o.res == o2.res, "the same call gave other values");
    // centred: against the eigenvalues of J A J by Jacobi
    for (int64_t n : {2, 5, 50}) {
        std::vector<double> l(lam.begin(), lam.begin() + n);
        Host c = similar(l, rng, true);
        std::vector<double> b(n * n);
        std::vector<double> col(n, 0.0);
        double all = 0.0;
        for (int64_t i = 0; i < n; ++i)
            for (int64_t j = 0; j < n; ++j) { col[j] += c.a[i * n + j] / n; all += c.a[i * n + j] / (n * n); }
        for (int64_t i = 0; i < n; ++i)
            for (int64_t j = 0; j < n; ++j) b[i * n + j] = c.a[i * n + j] - col[i] - col[j] + all;
        const std::vector<double> ref = jacobi(b, n);
        const int k = static_cast<int>(std::min<int64_t>(n - 1, 4));
        Out oc = run(c, k, 1e-10, 300, 4);
        for (int i = 0; i < k; ++i) {
            CHECK(oc.rc == 0 && oc.conv[i] == 1 && std::fabs(oc.val[i] - ref[i]) <= oc.res[i] + 1e-13, "centred n = %ld: value %d = %.17g, Jacobi %.17g", (long)n, i, oc.val[i], ref[i]);
            double s = 0.0;
            for (int64_t r = 0; r < n; ++r) s += oc.vec[r * k + i];
            CHECK(std::fabs(s) <= 64.0 * n * U, "centred n = %ld: vector %d sums to %g", (long)n, i, s);
        }
    }
}

void non_finite_and_failures(std::mt19937_64 &rng)
{
    std::vector<double> lam(15);
    for (int i = 0; i < 15; ++i) lam[i] = 1.0 / (1 + i);
    for (double bad : {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()}) {
        Host m = similar(lam, rng);
        m.a[3 * 15 + 3] = bad;
        Out o = run(m, 3, 1e-8, 300, 1, false);
        CHECK(o.rc == 0 && o.prod >= 1, "non-finite: rc = %d, %d products", o.rc, o.prod);
        for (int c = 0; c < 3; ++c) CHECK(std::isnan(o.val[c]) && std::isnan(o.res[c]) && o.conv[c] == 0, "non-finite: pair %d = %g, residual %g, flag %d", c, o.val[c], o.res[c], o.conv[c]);
        for (double e : o.vec) CHECK(std::isnan(e), "non-finite: a vector entry is %g", e);
    }
    Host m = similar(lam, rng);
    for (int op = 0; op < 9; ++op)
        for (long at : {0L, 2L}) {
            m.fail_op = op;
            m.fail_at = at;
            for (long &c : m.calls) c = 0;
            Out o = run(m, 3, 1e-10, 300, 1);
            const bool reached = m.calls[op] > at;           // (set and download are called once: their third call never comes)
            CHECK(o.rc == (reached ? 77 : 0), "failing op %d at call %ld: rc = %d", op, at, o.rc);
            if (o.rc) {
                CHECK(o.prod == -7, "a failed call wrote products");
                for (int c = 0; c < 3; ++c) CHECK(o.val[c] == kSentinel && o.res[c] == kSentinel && o.conv[c] == -7, "a failed call wrote pair %d", c);
                for (double e : o.vec) CHECK(e == kSentinel, "a failed call wrote a vector");
            }
        }
}

void tridiagonal_against_jacobi(std::mt19937_64 &rng)
{
    std::uniform_real_distribution<double> uni(-1.0, 1.0);
    for (int n = 1; n <= 40; ++n)
        for (int rep = 0; rep < 3; ++rep) {
            std::vector<double> d(n), e(n, 0.0), dense(n * n, 0.0);
            for (int i = 0; i < n; ++i) d[i] = rep == 2 ? 0.5 : uni(rng);
            for (int i = 0; i + 1 < n; ++i) e[i] = (rep >= 1 && i % 3 == 1) ? 0.0 : uni(rng);      // zeros: the places of breakdowns
            for (int i = 0; i < n; ++i) {
                dense[i * n + i] = d[i];
                if (i + 1 < n) dense[i * n + i + 1] = dense[(i + 1) * n + i] = e[i];
            }
            std::vector<double> d1 = d, e1 = e, z(n * n, 0.0), d2 = d, e2 = e, last(n, 0.0);
            for (int i = 0; i < n; ++i) z[i * n + i] = 1.0;
            last[n - 1] = 1.0;
            CHECK(genphi::tridiagonal_ql(n, d1.data(), e1.data(), z.data(), n), "QL failed, n = %d", n);
            CHECK(genphi::tridiagonal_ql(n, d2.data(), e2.data(), last.data(), 1), "QL failed, n = %d", n);
            for (int i = 0; i < n; ++i) {
                CHECK(d1[i] == d2[i] && last[i] == z[(n - 1) * n + i], "the one-row pass differs from the full one at %d of %d", i, n);
                double rr = 0.0, zz = 0.0;                   // T z_i = d_i z_i, |z_i| = 1
                for (int r = 0; r < n; ++r) {
                    double s = 0.0;
                    for (int c = 0; c < n; ++c) s += dense[r * n + c] * z[c * n + i];
                    rr += (s - d1[i] * z[r * n + i]) * (s - d1[i] * z[r * n + i]);
                    zz += z[r * n + i] * z[r * n + i];
                }
                CHECK(std::sqrt(rr) <= 64.0 * n * U * 3.0 && std::fabs(zz - 1.0) <= 64.0 * n * U, "n = %d eigenvector %d: residual %g, norm^2 - 1 = %g", n, i, std::sqrt(rr), zz - 1.0);
            }
            std::vector<double> got = d1;
            std::sort(got.begin(), got.end(), [](double x, double y) { return x > y; });
            const std::vector<double> ref = jacobi(dense, n);
            for (int i = 0; i < n; ++i) CHECK(std::fabs(got[i] - ref[i]) <= 64.0 * n * U * 3.0, "n = %d eigenvalue %d: QL %.17g, Jacobi %.17g", n, i, got[i], ref[i]);
            ++matrices;
        }
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20261019);
    tridiagonal_against_jacobi(rng);
    known_spectra(rng);
    multiple_and_invariant(rng);
    limits_and_centring(rng);
    non_finite_and_failures(rng);
    std::printf("eigen check: %ld matrices, %ld pairs, %ld products; %d violations\n", matrices, pairs, products, violations);
    return violations ? 1 : 0;
}
