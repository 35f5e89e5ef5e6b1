// Stand-alone check of csrc/f64_geometry.h, without a GPU (tests/test_f64_geometry_host.py builds and runs it): over every source cut of
// 0 .. 21,000 members, with the row pitch the plan gives a cut of that size and with pitches up to 45,056, for 1, 7 and 100,000 rows, 1
// and 256 CUs, both kernel settings and four LDS budgets, the geometry of a Float64 level launch
//   - takes the form the budget allows (the boundaries at the default budget are spelled out),
//   - covers the staged source row(s) with the kernel's per-thread pieces and the output row with its per-thread columns,
//   - keeps every source index within the 16 bits the full / split kernels pack it into,
//   - fits the LDS budget, and launches between 1 and rows_n persistent workgroups.
// A wrong block size here is a silently wrong kinship, not a crash: level_full64_kernel stages at most 2 * block * kF64Pre doubles.
#include <cstdio>
#include <initializer_list>

#include "../genlib.jl_amd/csrc/f64_geometry.h"

using namespace genphi;

static long long g_checks = 0, g_violations = 0;
static long long g_forms[3] = {0, 0, 0};

static void violation(const char *what, long long a, long long b, long long c, long long d)
{
    if (++g_violations <= 5) std::fprintf(stderr, "VIOLATION: %s (%lld, %lld, %lld, %lld)\n", what, a, b, c, d);
}
#define CHECK(cond, what, a, b, c, d) do { ++g_checks; if (!(cond)) violation(what, a, b, c, d); } while (0)

static long long pitch_for(long long n) { return ((n + 1) + 63) / 64 * 64; }      // (planner.h)

static void check_one(long long n_prev, long long ld, int rows_n, int n_cus, int kernel, size_t budget)
{
    const F64Geometry g = f64_geometry(n_prev, ld, rows_n, n_cus, kernel, budget);
    const long long lds_row = (n_prev + 2) / 2 * 2, b = static_cast<long long>(budget);
    CHECK(g.lds_row == lds_row && g.lds_row >= n_prev + 1, "lds_row", g.lds_row, lds_row, n_prev, 0);
    // the form: the first of full / split that the budget, the 16-bit index pack and the caller allow
    const bool rows_kernel = kernel != 1 && rows_n > 0;
    const F64Form want = rows_kernel && 2 * lds_row * 8 <= b ? kF64Full : (rows_kernel && lds_row * 8 <= b && n_prev < 65535 ? kF64Split : kF64Naive);
    CHECK(g.form == want, "form", g.form, want, n_prev, b);
    ++g_forms[g.form];
    if (g.form == kF64Full) {
        CHECK(g.block == 64 || g.block == 256 || g.block == 512, "full: block", g.block, n_prev, ld, 0);
        CHECK(g.lds_bytes == static_cast<size_t>(2 * lds_row * 8) && g.lds_bytes <= budget, "full: LDS bytes", static_cast<long long>(g.lds_bytes), lds_row, b, 0);
        CHECK(lds_row <= 2LL * g.block * kF64Pre, "full: the staging loop does not cover the row", lds_row, g.block, kF64Pre, ld);
        CHECK(static_cast<long long>(g.grid_y) * g.block * kF64Cols >= ld, "full: the chunks do not cover the columns", g.grid_y, g.block, ld, n_prev);
        CHECK(n_prev + 1 <= 65536, "full: a source index does not fit 16 bits", n_prev, 0, 0, 0);
        CHECK(g.grid_x >= 1 && g.grid_x <= rows_n, "full: grid.x", g.grid_x, rows_n, n_cus, g.grid_y);
        const bool fits64 = ld <= 64 * kF64Cols && lds_row <= 128 * kF64Pre, fits256 = ld <= 256 * kF64Cols && lds_row <= 512 * kF64Pre;
        CHECK((g.block == 64) == fits64, "full: block 64 exactly when the row and the columns fit it", g.block, ld, lds_row, 0);
        CHECK((g.block == 256) == (!fits64 && fits256), "full: block 256 exactly when they fit it and not 64", g.block, ld, lds_row, 0);
    } else if (g.form == kF64Split) {
        CHECK(g.block == 512, "split: block", g.block, 0, 0, 0);
        CHECK(g.lds_bytes == static_cast<size_t>(lds_row * 8) && g.lds_bytes <= budget, "split: LDS bytes", static_cast<long long>(g.lds_bytes), lds_row, b, 0);
        CHECK(lds_row <= 2LL * 512 * kS64Pre, "split: the staging loop does not cover the row", lds_row, kS64Pre, 0, 0);
        CHECK(n_prev < 65535, "split: a source index does not fit 16 bits", n_prev, 0, 0, 0);
        CHECK(static_cast<long long>(g.grid_y) * 512 * kS64Cols >= ld, "split: the chunks do not cover the columns", g.grid_y, ld, n_prev, 0);
        CHECK(g.grid_x >= 1 && g.grid_x <= rows_n, "split: grid.x", g.grid_x, rows_n, n_cus, g.grid_y);
    } else {
        CHECK(g.block == 256 && g.lds_bytes == 0, "naive: block / LDS", g.block, static_cast<long long>(g.lds_bytes), 0, 0);
        CHECK(g.grid_x == rows_n && g.grid_y == (ld + 255) / 256, "naive: the grid is rows_n x ceil(ld / 256)", g.grid_x, g.grid_y, rows_n, ld);
    }
}

static void check_inputs(long long n_prev, long long ld)
{
    for (int rows_n : {1, 7, 100000})
        for (int n_cus : {1, 256})
            for (size_t budget : {size_t(160 * 1024), size_t(4 * 300), size_t(4 * 2048), size_t(4 * 8192)}) {
                check_one(n_prev, ld, rows_n, n_cus, 0, budget);
                check_one(n_prev, ld, rows_n, n_cus, 1, budget);
            }
    check_one(n_prev, ld, 0, 256, 0, 160 * 1024);
}

int main()
{
    // the budget rule: 160 KB, or four bytes per float of the GENPHI_LDS_CAP_FLOATS hook when that is at least 16, whichever is smaller
    CHECK(f64_lds_budget(0) == 163840 && f64_lds_budget(15) == 163840 && f64_lds_budget(-1) == 163840, "budget: hook unset", 0, 0, 0, 0);
    CHECK(f64_lds_budget(16) == 64 && f64_lds_budget(300) == 1200 && f64_lds_budget(40960) == 163840 && f64_lds_budget(40961) == 163840 &&
          f64_lds_budget(1 << 30) == 163840, "budget: hook set", 0, 0, 0, 0);
    // the form boundaries at the default budget: lds_row = (n_prev + 2) / 2 * 2 doubles, 163,840 bytes
    const size_t dflt = f64_lds_budget(0);
    const struct { long long n_prev; int rows_n, kernel; F64Form form; } edges[] = {
        {10239, 7, 0, kF64Full}, {10240, 7, 0, kF64Split}, {20479, 7, 0, kF64Split}, {20480, 7, 0, kF64Naive},
        {100, 7, 1, kF64Naive}, {100, 0, 0, kF64Naive}, {15000, 7, 1, kF64Naive}, {15000, 0, 0, kF64Naive}, {0, 1, 0, kF64Full}};
    for (const auto &e : edges)
        CHECK(f64_geometry(e.n_prev, pitch_for(e.n_prev), e.rows_n, 256, e.kernel, dflt).form == e.form, "form boundary", e.n_prev, e.rows_n, e.kernel, e.form);
    // every source cut with the pitch of a cut of that size, then pitches up to the widest result the delivery serves in one chunk
    for (long long n_prev = 0; n_prev <= 21000; ++n_prev) check_inputs(n_prev, pitch_for(n_prev));
    for (long long n_prev = 0; n_prev <= 21000; ++n_prev)
        for (long long ld : {64LL, 1280LL, 1344LL, 5120LL, 5184LL, 7168LL, 7232LL, 10240LL, 10304LL, 14336LL, 14400LL, 21056LL, 45056LL})
            check_inputs(n_prev, ld);
    std::printf("f64 geometry check: %lld checks, %lld full, %lld split and %lld naive launches; %lld violations\n", g_checks, g_forms[0], g_forms[1],
                g_forms[2], g_violations);
    return g_violations ? 1 : 0;
}
