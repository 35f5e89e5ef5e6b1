// solve_check.cpp -- the conjugate-gradient core of genphi_result_solve (csrc/result_solve.cpp: genphi::cg_solve) without a GPU: a
// stand-alone program that hands it a host product over a dense Float64 matrix and checks what include/genphi.h promises of the
// iteration.  Built by tests/test_solve_host.py with g++, once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer.
//
// Matrices with a known spectrum: A = H D H, H = I - 2 v v^T / (v^T v) a Householder reflection, D = diag(lam).  The bounds:
//   iterations <= ceil(ln(tol / (2 sqrt(kappa))) / ln((sqrt(kappa) - 1) / (sqrt(kappa) + 1))) + 1     (the classical CG bound carried
//                 to the residual norm, kappa = lam_max / lam_min of the spectrum the matrix was built from: the rounding of H D H
//                 moves an eigenvalue by the order of n u lam_max, which no case here turns into another ceiling)
//   |reported residual - recomputed residual| <= rounding = 2 (n + 2) u || |A| |z| + |b| || / ||b||,  u = 2^-53
//   reported residual <= tol + (iterations + 1) rounding for a column that stopped by its recurrence residual: the recurrence and the
//                 true residual part by at most one product's rounding per step (the iterates' norms grow monotonically from z = 0)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../genlib.jl_amd/csrc/result_solve.h"

namespace {

int violations = 0;
long systems = 0, columns = 0, products = 0;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            ++violations;                                  \
            std::fprintf(stderr, "VIOLATION %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);             \
            std::fprintf(stderr, "\n");                    \
        }                                                  \
    } while (0)

struct Dense {
    int64_t n;
    std::vector<double> a;                                  // n x n row-major
    std::vector<int> widths;                                // kk of every product
    genphi::CgProduct product()
    {
        return [this](int32_t kk, const double *x, double *y) {
            widths.push_back(kk);
            ++products;
            for (int64_t i = 0; i < n; ++i)
                for (int32_t c = 0; c < kk; ++c) {
                    double s = 0.0;
                    for (int64_t j = 0; j < n; ++j) s += a[i * n + j] * x[j * kk + c];
                    y[i * kk + c] = s;
                }
            return 0;
        };
    }
};

Dense spd(int64_t n, double lam_min, double lam_max, std::mt19937_64 &rng)
{
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    std::normal_distribution<double> nor;
    std::vector<double> lam(n), v(n);
    double vv = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        lam[i] = i == 0 ? lam_min : i == n - 1 ? lam_max : lam_min + (lam_max - lam_min) * uni(rng);
        v[i] = nor(rng);
        vv += v[i] * v[i];
    }
    Dense m{n, std::vector<double>(n * n), {}};
    // A = H D H, entry (i, j) = sum_l H_il lam_l H_lj
    std::vector<double> h(n * n);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < n; ++j) h[i * n + j] = (i == j ? 1.0 : 0.0) - 2.0 * v[i] * v[j] / vv;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int64_t l = 0; l < n; ++l) s += h[i * n + l] * lam[l] * h[l * n + j];
            m.a[i * n + j] = m.a[j * n + i] = s;
        }
    return m;
}

int iteration_bound(double kappa, double tol)
{
    const double s = std::sqrt(kappa);
    if (s <= 1.0) return 2;
    return static_cast<int>(std::ceil(std::log(tol / (2.0 * s)) / std::log((s - 1.0) / (s + 1.0)))) + 1;
}

// recomputed relative residual of column c and the rounding term
void residual_of(const Dense &m, double ridge, const double *b, int64_t ldb, const double *z, int64_t ldz, int c, double *res, double *rounding)
{
    const int64_t n = m.n;
    double rr = 0.0, bb = 0.0, mag = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        double s = 0.0, t = 0.0;
        for (int64_t j = 0; j < n; ++j) {
            const double a = m.a[i * n + j] + (i == j ? ridge : 0.0);
            s += a * z[j * ldz + c];
            t += std::fabs(a) * std::fabs(z[j * ldz + c]);
        }
        const double e = b[i * ldb + c] - s;
        rr += e * e;
        bb += b[i * ldb + c] * b[i * ldb + c];
        t += std::fabs(b[i * ldb + c]);
        mag += t * t;
    }
    *res = std::sqrt(rr) / std::sqrt(bb);
    *rounding = 2.0 * (n + 2) * std::ldexp(1.0, -53) * std::sqrt(mag) / std::sqrt(bb);
}

constexpr double kSentinel = -7.0;

// one system with pitches beyond k; checks everything that holds for every SPD system, returns the outputs (dense)
struct Out { std::vector<double> z, res; std::vector<int32_t> its; };
Out solve_and_check(Dense &m, int k, const std::vector<double> &b_dense, double ridge, double tol, int max_iter, double kappa, bool expect_converged)
{
    const int64_t n = m.n, ldb = k + 2, ldz = k + 3;
    std::vector<double> b(n * ldb, std::numeric_limits<double>::quiet_NaN()), z(n * ldz, kSentinel), res(k, kSentinel);
    std::vector<int32_t> its(k, -7);
    for (int64_t i = 0; i < n; ++i)
        for (int c = 0; c < k; ++c) b[i * ldb + c] = b_dense[i * k + c];
    m.widths.clear();
    const int rc = genphi::cg_solve(n, k, b.data(), ldb, ridge, tol, max_iter, m.product(), z.data(), ldz, res.data(), its.data());
    CHECK(rc == 0, "cg_solve returned %d", rc);
    ++systems;
    columns += k;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t g = k; g < ldz; ++g) CHECK(z[i * ldz + g] == kSentinel, "the gap of z was written at row %ld", (long)i);
    // the products: widths never grow during the iteration, their sum is the sum of the iteration counts; one more for the residual
    long sum_its = 0, sum_w = 0;
    int nonzero = 0;
    for (int c = 0; c < k; ++c) {
        sum_its += its[c];
        bool any = false;
        for (int64_t i = 0; i < n; ++i) any = any || b_dense[i * k + c] != 0.0;
        nonzero += any ? 1 : 0;
    }
    const size_t n_cg = m.widths.size() - (nonzero ? 1 : 0);
    for (size_t w = 0; w < n_cg; ++w) {
        sum_w += m.widths[w];
        if (w) CHECK(m.widths[w] <= m.widths[w - 1], "product %zu took %d columns after %d", w, m.widths[w], m.widths[w - 1]);
    }
    CHECK(sum_w == sum_its, "the products took %ld columns, the iteration counts add up to %ld", sum_w, sum_its);
    CHECK(!nonzero || m.widths.back() == nonzero, "the residual product took %d columns, %d are not zero", m.widths.empty() ? -1 : m.widths.back(), nonzero);
    CHECK(static_cast<long>(n_cg) <= max_iter, "%zu products with max_iter = %d", n_cg, max_iter);
    const int cap = iteration_bound(kappa, tol);
    Out o{std::vector<double>(n * k), res, its};
    for (int c = 0; c < k; ++c) {
        for (int64_t i = 0; i < n; ++i) o.z[i * k + c] = z[i * ldz + c];
        bool any = false;
        for (int64_t i = 0; i < n; ++i) any = any || b_dense[i * k + c] != 0.0;
        if (!any) {
            CHECK(its[c] == 0 && res[c] == 0.0, "zero column %d: %d iterations, residual %g", c, its[c], res[c]);
            for (int64_t i = 0; i < n; ++i) CHECK(z[i * ldz + c] == 0.0, "zero column %d has a solution entry %g", c, z[i * ldz + c]);
            continue;
        }
        CHECK(its[c] >= 1 && its[c] <= max_iter, "column %d: %d iterations", c, its[c]);
        double want, rounding;
        residual_of(m, ridge, b.data(), ldb, z.data(), ldz, c, &want, &rounding);
        CHECK(std::fabs(res[c] - want) <= rounding, "column %d: residual %g, recomputed %g, rounding %g", c, res[c], want, rounding);
        if (expect_converged) {
            CHECK(res[c] <= tol + (its[c] + 1) * rounding, "column %d: residual %g above tol %g (n %ld, kappa %g)", c, res[c], tol, (long)n, kappa);
            CHECK(its[c] <= cap, "column %d: %d iterations, the bound is %d (n %ld, kappa %g)", c, its[c], cap, (long)n, kappa);
        }
    }
    return o;
}

std::vector<double> normal_rhs(int64_t n, int k, std::mt19937_64 &rng)
{
    std::normal_distribution<double> nor;
    std::vector<double> b(n * k);
    for (double &x : b) x = nor(rng);
    return b;
}

std::vector<double> column(const std::vector<double> &a, int64_t n, int k, int c)
{
    std::vector<double> out(n);
    for (int64_t i = 0; i < n; ++i) out[i] = a[i * k + c];
    return out;
}

void spd_systems(std::mt19937_64 &rng)
{
    const int64_t sizes[] = {1, 2, 3, 7, 50, 200};
    const double kappas[] = {1.0, 3.0, 100.0, 1.0e4};
    for (int64_t n : sizes)
        for (double kappa : kappas)
            for (double ridge : {0.0, 0.5}) {
                if (n == 1 && kappa != 1.0) continue;
                Dense m = spd(n, 0.25, 0.25 * kappa, rng);
                const double kap = (0.25 * kappa + ridge) / (0.25 + ridge), tol = 1e-10;
                const int k = 8;
                std::vector<double> b = normal_rhs(n, k, rng);
                for (int64_t i = 0; i < n; ++i) { b[i * k + 6] = 1.0; b[i * k + 7] = 0.0; }
                for (int64_t i = 0; i < n; ++i) b[i * k + 5] *= 1.0e-100;                  // a tiny column: its own scale
                const Out all = solve_and_check(m, k, b, ridge, tol, 5000, kap, true);
                // every column alone gives the column's bytes: its scalars are its own, and a column that stopped is not touched again
                for (int c = 0; c < k; ++c) {
                    const Out one = solve_and_check(m, 1, column(b, n, k, c), ridge, tol, 5000, kap, true);
                    CHECK(one.its[0] == all.its[c] && std::memcmp(&one.res[0], &all.res[c], sizeof(double)) == 0, "column %d alone: %d iterations, %d in company", c,
                          one.its[0], all.its[c]);
                    const std::vector<double> zc = column(all.z, n, k, c);
                    CHECK(std::memcmp(one.z.data(), zc.data(), n * sizeof(double)) == 0, "column %d alone has another solution (n %ld)", c, (long)n);
                }
                // the same call, the same bits
                const Out again = solve_and_check(m, k, b, ridge, tol, 5000, kap, true);
                CHECK(std::memcmp(again.z.data(), all.z.data(), all.z.size() * sizeof(double)) == 0 && again.its == all.its, "the same call gave other bits");
                // max_iter = 1: one product each, nothing converged at kappa > 1, still the residual of what there is
                const Out cut = solve_and_check(m, k, b, ridge, tol, 1, kap, false);
                for (int c = 0; c < 7; ++c) {
                    CHECK(cut.its[c] == 1, "max_iter = 1: column %d made %d products", c, cut.its[c]);
                    if (kappa > 1.0 && n > 1 && c < 5) CHECK(cut.res[c] > tol, "max_iter = 1: column %d already at %g", c, cut.res[c]);
                }
            }
}

void breakdowns(std::mt19937_64 &rng)
{
    const double tol = 1e-10;
    // a singular matrix: diag(1, 0) and b = (1, 1): one step along (1, 1), then d = (0, 2) has no curvature; the column stops with z = (2, 2)
    {
        Dense m{2, {1.0, 0.0, 0.0, 0.0}, {}};
        double b[2] = {1.0, 1.0}, z[2] = {kSentinel, kSentinel}, res = kSentinel;
        int32_t its = -7;
        const int rc = genphi::cg_solve(2, 1, b, 1, 0.0, tol, 1000, m.product(), z, 1, &res, &its);
        ++systems; ++columns;
        CHECK(rc == 0 && its == 2 && z[0] == 2.0 && z[1] == 2.0, "singular: rc %d, %d iterations, z = (%g, %g)", rc, its, z[0], z[1]);
        CHECK(std::fabs(res - 1.0) < 1e-15, "singular: residual %g", res);                       // r = (-1, 1) over ||b|| = sqrt 2
        CHECK(m.widths.size() == 3, "singular: %zu products", m.widths.size());
    }
    // b in the null space: no curvature at once: z = 0, one product, residual 1
    {
        Dense m{2, {1.0, 0.0, 0.0, 0.0}, {}};
        double b[2] = {0.0, 3.0}, z[2] = {kSentinel, kSentinel}, res = kSentinel;
        int32_t its = -7;
        const int rc = genphi::cg_solve(2, 1, b, 1, 0.0, tol, 1000, m.product(), z, 1, &res, &its);
        ++systems; ++columns;
        CHECK(rc == 0 && its == 1 && z[0] == 0.0 && z[1] == 0.0 && res == 1.0, "null space: rc %d, %d iterations, z = (%g, %g), residual %g", rc, its, z[0], z[1], res);
    }
    // ... which a ridge repairs: (0 + 0.5) z = 3
    {
        Dense m{2, {1.0, 0.0, 0.0, 0.0}, {}};
        double b[2] = {0.0, 3.0}, z[2], res;
        int32_t its;
        const int rc = genphi::cg_solve(2, 1, b, 1, 0.5, tol, 1000, m.product(), z, 1, &res, &its);
        ++systems; ++columns;
        CHECK(rc == 0 && its == 1 && z[0] == 0.0 && z[1] == 6.0 && res == 0.0, "ridge: rc %d, %d iterations, z = (%g, %g), residual %g", rc, its, z[0], z[1], res);
    }
    // a negative definite matrix: negative curvature stops every column at its first product
    {
        Dense m = spd(20, 1.0, 5.0, rng);
        for (double &a : m.a) a = -a;
        const std::vector<double> b = normal_rhs(20, 3, rng);
        std::vector<double> z(60, kSentinel), res(3);
        std::vector<int32_t> its(3);
        const int rc = genphi::cg_solve(20, 3, b.data(), 3, 0.0, tol, 1000, m.product(), z.data(), 3, res.data(), its.data());
        ++systems; columns += 3;
        CHECK(rc == 0 && its[0] == 1 && its[1] == 1 && its[2] == 1, "negative definite: rc %d, iterations %d %d %d", rc, its[0], its[1], its[2]);
        for (double x : z) CHECK(x == 0.0, "negative definite: a solution entry %g", x);
        for (double r : res) CHECK(r == 1.0, "negative definite: residual %g", r);
    }
    // a NaN in one right-hand side, an inf in another, a NaN in the matrix: those columns stop cleanly, the others are what they are alone
    for (int where = 0; where < 2; ++where) {
        const int64_t n = 30;
        const int k = 4;
        Dense m = spd(n, 0.5, 4.0, rng);
        std::vector<double> b = normal_rhs(n, k, rng);
        const Out clean = solve_and_check(m, k, b, 0.25, tol, 1000, 4.25 / 0.75, true);
        if (where == 0) {
            b[7 * k + 1] = std::numeric_limits<double>::quiet_NaN();
            b[9 * k + 3] = std::numeric_limits<double>::infinity();
            std::vector<double> z(n * k, kSentinel), res(k, kSentinel);
            std::vector<int32_t> its(k, -7);
            const int rc = genphi::cg_solve(n, k, b.data(), k, 0.25, tol, 1000, m.product(), z.data(), k, res.data(), its.data());
            ++systems; columns += k;
            CHECK(rc == 0, "NaN in b: rc %d", rc);
            CHECK(its[1] == 1 && std::isnan(res[1]), "NaN column: %d iterations, residual %g", its[1], res[1]);
            CHECK(its[3] <= 1 && !(res[3] <= tol), "inf column: %d iterations, residual %g", its[3], res[3]);
            for (int64_t i = 0; i < n; ++i) CHECK(z[i * k + 1] == 0.0 && z[i * k + 3] == 0.0, "a column that broke down has a solution entry at row %ld", (long)i);
            for (int c : {0, 2}) {
                CHECK(its[c] == clean.its[c] && std::memcmp(&res[c], &clean.res[c], sizeof(double)) == 0, "column %d changed beside a NaN column", c);
                for (int64_t i = 0; i < n; ++i) CHECK(std::memcmp(&z[i * k + c], &clean.z[i * k + c], sizeof(double)) == 0, "column %d, row %ld changed beside a NaN column", c, (long)i);
            }
        } else {
            m.a[3 * n + 3] = std::numeric_limits<double>::quiet_NaN();
            std::vector<double> z(n * k, kSentinel), res(k, kSentinel);
            std::vector<int32_t> its(k, -7);
            const int rc = genphi::cg_solve(n, k, b.data(), k, 0.25, tol, 1000, m.product(), z.data(), k, res.data(), its.data());
            ++systems; columns += k;
            CHECK(rc == 0, "NaN in the matrix: rc %d", rc);
            for (int c = 0; c < k; ++c) {
                CHECK(its[c] == 1 && std::isnan(res[c]), "NaN in the matrix: column %d made %d products, residual %g", c, its[c], res[c]);
                for (int64_t i = 0; i < n; ++i) CHECK(z[i * k + c] == 0.0, "NaN in the matrix: a solution entry at row %ld", (long)i);
            }
        }
    }
    // a product that fails: its code comes back and nothing is written
    {
        double b[2] = {1.0, 2.0}, z[2] = {kSentinel, kSentinel}, res = kSentinel;
        int32_t its = -7;
        const int rc = genphi::cg_solve(2, 1, b, 1, 0.0, tol, 10, [](int32_t, const double *, double *) { return 5; }, z, 1, &res, &its);
        CHECK(rc == 5 && z[0] == kSentinel && z[1] == kSentinel && res == kSentinel && its == -7, "a failing product: rc %d", rc);
    }
    // residual and iterations may be NULL
    {
        Dense m{1, {2.0}, {}};
        double b = 3.0, z = kSentinel;
        const int rc = genphi::cg_solve(1, 1, &b, 1, 0.0, tol, 10, m.product(), &z, 1, nullptr, nullptr);
        CHECK(rc == 0 && z == 1.5, "1 x 1: rc %d, z %g", rc, z);
    }
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20261018);
    spd_systems(rng);
    breakdowns(rng);
    std::printf("solve check: %ld systems, %ld columns, %ld products; %d violations\n", systems, columns, products, violations);
    return violations ? 1 : 0;
}
