// link_check.cpp -- the host side of gen.simuSharing (csrc/link.cpp, csrc/link.h) as a stand-alone program: built by
// tests/test_link_host.py with g++, plain and under AddressSanitizer + UndefinedBehaviorSanitizer, together with link.cpp, ident.cpp,
// pedigree_index.cpp, ancestor_sweep.cpp and planner.cpp.  The crossover and transmission words of link_words are checked against the
// definition in include/genphi.h restated here bit by bit (all sixteen words of the fold, a running parity), the shapes and the device
// sizes of link.h against their formulas on random plans, and genphi_link_words' refusals.  Prints one summary line; exit status 1 on
// any violation.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../genlib.jl_amd/csrc/link.h"
#include "../include/genphi.h"

int genphi_set_error(int code, const std::string &) { return code; }      // (the library's is in genphi_hip.hip)

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
int64_t below(int64_t n) { return static_cast<int64_t>(rnd() % static_cast<uint64_t>(n)); }

long violations = 0;
void expect(bool ok, const char *what, long at)
{
    if (ok) return;
    ++violations;
    std::fprintf(stderr, "VIOLATION in case %ld: %s\n", at, what);
}

// the definition, one bit at a time
void literal(uint64_t seed, int64_t id, int side, uint32_t s, int L, int q, std::vector<int> &x, std::vector<int> &t)
{
    const uint64_t uid = static_cast<uint64_t>(id);
    const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
    x.assign(L, 0);
    t.assign(L, 0);
    for (int w = 0; 64 * w < L; ++w) {
        uint64_t acc = 0;
        for (int tt = 0; tt < 16; ++tt) {
            const uint32_t c3 = 0x80000000u | static_cast<uint32_t>(side) | (static_cast<uint32_t>(w) << 1) | (static_cast<uint32_t>(tt / 2) << 8);
            const genphi::PhiloxPair u = genphi::philox_pair(static_cast<uint32_t>(uid), static_cast<uint32_t>(uid >> 32), s, c3, k0, k1);
            const uint64_t U = tt % 2 ? u.w1 : u.w0;
            acc = (q >> tt) & 1 ? (acc | U) : (acc & U);
        }
        for (int k = 0; k < 64 && 64 * w + k < L; ++k) x[64 * w + k] = static_cast<int>((acc >> k) & 1);
    }
    const genphi::PhiloxPair u = genphi::philox_pair(static_cast<uint32_t>(uid), static_cast<uint32_t>(uid >> 32), s, 0x80000000u | static_cast<uint32_t>(side) | (8u << 8), k0, k1);
    x[0] = static_cast<int>(u.w0 & 1);
    int parity = 0;
    for (int k = 0; k < L; ++k) {
        parity ^= x[k];
        t[k] = parity;
    }
}

}  // namespace

int main()
{
    long cases = 0, loci = 0, crossovers = 0, refusals = 0, plans = 0;
    const int Ls[] = {1, 2, 63, 64, 65, 127, 128, 129, 191, 1000, 4095, 4096};
    const int qs[] = {0, 1, 2, 64, 0x5555, 0x8000 - 1, 0x8000, 12345, 0x4000, 3};
    std::vector<int> x, t;
    for (int L : Ls)
        for (int q : qs)
            for (int rep = 0; rep < 4; ++rep) {
                const uint64_t seed = rnd();
                const int64_t id = rep == 0 ? 1 : (rep == 1 ? -7 : static_cast<int64_t>(rnd() >> (rep == 2 ? 1 : 40)));
                const int side = static_cast<int>(below(2));
                const uint32_t s = static_cast<uint32_t>(below(1 << 24));
                const genphi::LinkShape z = genphi::link_shape(L, q);
                expect(z.L == L && z.q == q && z.W == (L + 63) / 64 && z.Wp == (z.W + 1) / 2 && z.lanes >= z.Wp && z.lanes <= 32 && (z.lanes & (z.lanes - 1)) == 0 &&
                           (z.lanes == 1 || z.lanes / 2 < z.Wp),
                       "link_shape", cases);
                std::vector<uint64_t> X(z.W, 0xDEADull), T(z.W, 0xBEEFull), X2(z.W), T2(z.W);
                genphi::link_words(seed, id, side, s, z, X.data(), T.data());
                expect(genphi_link_words(seed, id, side, s, L, q, X2.data(), T2.data()) == GENPHI_OK && X2 == X && T2 == T, "genphi_link_words", cases);
                genphi::link_words(seed, id, side, s, z, nullptr, T2.data());
                genphi::link_words(seed, id, side, s, z, X2.data(), nullptr);
                expect(X2 == X && T2 == T, "NULL outputs", cases);
                literal(seed, id, side, s, L, q, x, t);
                bool same = true;
                for (int k = 0; k < L; ++k) {
                    same = same && static_cast<int>((X[k / 64] >> (k % 64)) & 1) == x[k] && static_cast<int>((T[k / 64] >> (k % 64)) & 1) == t[k];
                    crossovers += k > 0 && x[k];
                }
                expect(same, "words against the definition", cases);
                int blocks = 0;                  // the blocks from the one that holds the lowest set bit of q
                for (int d = 0; d < 8; ++d)
                    if (q & ((1 << (2 * d + 2)) - 1)) ++blocks;
                expect(genphi::link_first_block(static_cast<uint32_t>(q)) == 8 - blocks && genphi::link_blocks_per_side(z) == static_cast<int64_t>(z.W) * blocks + 1,
                       "blocks drawn", cases);
                loci += L;
                ++cases;
            }
    uint64_t w = 0x8000000000000001ull;
    expect(genphi::link_prefix_xor(0) == 0 && genphi::link_prefix_xor(1) == ~0ull && genphi::link_prefix_xor(w) == 0x7FFFFFFFFFFFFFFFull &&
               genphi::link_prefix_xor(0x6ull) == 0x2ull,
           "prefix", -1);
    // ---- refusals ----
    uint64_t X1[64], T1[64];
    refusals += genphi_link_words(1, 1, 0, 0, 0, 64, X1, T1) == GENPHI_ERR_ARG;
    refusals += genphi_link_words(1, 1, 0, 0, 4097, 64, X1, T1) == GENPHI_ERR_ARG;
    refusals += genphi_link_words(1, 1, 0, 0, 64, -1, X1, T1) == GENPHI_ERR_ARG;
    refusals += genphi_link_words(1, 1, 0, 0, 64, 32769, X1, T1) == GENPHI_ERR_ARG;
    refusals += genphi_link_words(1, 1, 2, 0, 64, 64, X1, T1) == GENPHI_ERR_ARG;
    refusals += genphi_link_words(1, 1, -1, 0, 64, 64, X1, T1) == GENPHI_ERR_ARG;
    refusals += genphi_link_words(1, 1, 0, -1, 64, 64, X1, T1) == GENPHI_ERR_ARG;
    refusals += genphi_link_words(1, 1, 0, int64_t(1) << 24, 64, 64, X1, T1) == GENPHI_ERR_ARG;
    expect(genphi_link_words(1, 1, 1, (int64_t(1) << 24) - 1, 4096, 32768, X1, T1) == GENPHI_OK, "the largest arguments", -2);
    // ---- device sizes on random plans ----
    for (long ped = 0; ped < 300; ++ped) {
        const int64_t n = 2 + below(150);
        std::vector<int64_t> ind(n), fa(n, 0), mo(n, 0);
        for (int64_t i = 0; i < n; ++i) ind[i] = i + 1;
        for (int64_t i = 1; i < n; ++i) {
            const int64_t r = below(100);
            if (r < 15) continue;
            const int64_t f = below(i), m = below(i);
            if (r < 25) fa[i] = ind[f];
            else if (r < 35) mo[i] = ind[m];
            else { fa[i] = ind[f]; mo[i] = ind[m]; }
        }
        const int64_t n_pro = 1 + below(10);
        std::vector<int64_t> pro(n_pro);
        for (auto &p : pro) p = ind[below(n)];
        genphi::IdentPlan pl;
        std::string err;
        if (genphi::plan_ident(pl, n, ind.data(), fa.data(), mo.data(), n_pro, pro.data(), err) != GENPHI_OK) { expect(false, "plan_ident", ped); continue; }
        const int L = Ls[ped % 12];
        const int64_t S = 1 + below(5000);
        const bool lab = ped % 2 == 0;
        const genphi::LinkShape z = genphi::link_shape(L, 64);
        const genphi::LinkSizes a = genphi::link_sizes(pl, S, z, lab);
        const size_t B = static_cast<size_t>(pl.planes), Wp = static_cast<size_t>(z.Wp);
        expect(a.sums == static_cast<size_t>(48 * n_pro * n_pro) && a.labels == (lab ? static_cast<size_t>(8 * n_pro * S * L) : 0u), "result bytes", ped);
        expect(a.lists == static_cast<size_t>(4 * (2 * pl.n_live + n_pro) + 8 * (pl.n_live + pl.n_labels)), "list bytes", ped);
        expect(a.sim_rows == 32 * B * Wp * static_cast<size_t>(pl.n_live) && a.sim_gather == 32 * B * Wp * static_cast<size_t>(n_pro), "panel bytes", ped);
        expect(a.panel(7) == 7 * (a.sim_rows + a.sim_gather) && a.fixed() == a.sums + a.labels + a.lists, "sums", ped);
        // one simulation of a panel row is Wp elements of 2 sides x B planes x 16 bytes, and a panel is whole simulations
        const genphi::IdentSizes b = genphi::ident_sizes(pl, 128, false);
        expect(a.sim_rows == b.pair_rows * Wp && a.sim_gather == b.pair_gather * Wp, "ident's element", ped);
        int64_t Sn = 0;
        const double one = static_cast<double>(a.panel(1));
        expect(genphi::drop_panel_fits(Sn, 128 * S, 0, 1e18, one) && Sn == S, "default panel", ped);
        expect(genphi::drop_panel_fits(Sn, 128 * S, 128 * 3, 1e18, one) && Sn == (S < 3 ? S : 3), "forced panel", ped);
        expect(genphi::drop_panel_fits(Sn, 128 * S, 0, 2.5 * one, one) && Sn == (S < 2 ? S : 2), "the widest that fits", ped);
        expect(!genphi::drop_panel_fits(Sn, 128 * S, 0, 0.5 * one, one), "nothing fits", ped);
        ++plans;
    }
    std::printf("link check: %ld cases, %ld loci, %ld crossovers, %ld refusals, %ld plans; %ld violations\n", cases, loci, crossovers, refusals, plans, violations);
    return violations ? 1 : 0;
}
