// retain_check.cpp -- the host side of gen.simuRetention (csrc/retain.h) as a stand-alone program: built by tests/test_retain_host.py
// with g++, plain and under AddressSanitizer + UndefinedBehaviorSanitizer.  retain.h is header-only, and its functions read the sizes
// of a plan alone, so the plans here are lists of random lengths.  Checked: retain_sizes against the byte counts restated here; the
// chunk rule at the word edges of a bitmap, at the default's edge and at 10^6 labels, for the default and for forced widths, by
// walking every chunk; the panel rule (drop_panel_fits with retain_sizes) on random rooms.  Prints one summary line; exit status 1 on
// any violation.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../genlib.jl_amd/csrc/retain.h"

namespace {

uint64_t rng_state = 0x2545F4914F6CDD1Dull;
uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
int64_t below(int64_t n) { return static_cast<int64_t>(rnd() % static_cast<uint64_t>(n)); }

long violations = 0;
void expect(bool ok, const char *what, long long at)
{
    if (ok) return;
    ++violations;
    std::fprintf(stderr, "VIOLATION at %lld: %s\n", at, what);
}

long chunk_cases = 0, chunks_walked = 0, split_borders = 0;

// One (n_labels, chunk_arg): the rule's numbers, and a walk over the chunks: they tile [0, n_labels), start at multiples of 32, and
// the halo bit of every chunk but the last lies inside the bitmap.
void check_chunks(int64_t n_labels, int64_t arg)
{
    const genphi::RetainChunks c = genphi::retain_chunks(n_labels, arg);
    const long long at = n_labels * 100000 + arg;
    ++chunk_cases;
    int64_t want = arg > 0 ? (arg + 31) / 32 * 32 : (n_labels <= 8192 ? n_labels : 8192);
    if (want > n_labels) want = n_labels;
    if (want > 16384) want = 16384;
    expect(c.chunk_labels == want, "chunk width", at);
    expect(c.chunk_labels >= 1 && c.chunk_labels <= n_labels && c.chunk_labels <= genphi::RETAIN_MAX_CHUNK, "chunk width range", at);
    expect(c.chunks == (n_labels + c.chunk_labels - 1) / c.chunk_labels, "chunk count", at);
    expect(c.bitmap_dwords == (c.chunk_labels + 1 + 31) / 32, "bitmap dwords hold LC + 1 bits", at);
    expect(c.stride % 2 == 1 && c.stride >= c.bitmap_dwords && c.stride <= c.bitmap_dwords + 1, "odd stride", at);
    expect(c.lds_bytes == 256u * static_cast<size_t>(c.stride) && c.lds_bytes <= 160u * 1024u, "LDS bytes", at);
    // 64 lanes at dword s * stride + d: 64 different banks modulo 32 within each half of the wave, and modulo 64 over the wave
    bool seen32[2][32] = {}, seen64[64] = {};
    bool clash = false;
    for (int s = 0; s < 64; ++s) {
        const int b32 = static_cast<int>((static_cast<int64_t>(s) * c.stride) % 32), b64 = static_cast<int>((static_cast<int64_t>(s) * c.stride) % 64);
        clash = clash || seen32[s / 32][b32] || seen64[b64];
        seen32[s / 32][b32] = seen64[b64] = true;
    }
    expect(!clash, "bank conflict", at);
    int64_t covered = 0;
    for (int64_t k = 0; k < c.chunks; ++k) {
        const int64_t l0 = k * c.chunk_labels, l1 = l0 + c.chunk_labels < n_labels ? l0 + c.chunk_labels : n_labels;
        expect(l0 % 32 == 0 && l0 == covered && l1 > l0, "chunks tile the table from multiples of 32", at);
        covered = l1;
        if (k + 1 < c.chunks) {
            expect((l1 - l0) / 32 < c.bitmap_dwords, "the halo bit lies in the bitmap", at);
            ++split_borders;
        }
        ++chunks_walked;
    }
    expect(covered == n_labels, "coverage", at);
}

}  // namespace

int main()
{
    // ---- the chunk rule ----
    for (int64_t n : {int64_t(2), int64_t(31), int64_t(32), int64_t(33), int64_t(63), int64_t(64), int64_t(65), int64_t(8191), int64_t(8192), int64_t(8193), int64_t(16383), int64_t(16384),
                      int64_t(16385), int64_t(16416), int64_t(1000000), int64_t(2147483647)})
        for (int64_t arg : {int64_t(0), int64_t(1), int64_t(31), int64_t(32), int64_t(33), int64_t(64), int64_t(4096), int64_t(8192), int64_t(16383),
                            int64_t(16384), int64_t(16385), int64_t(2147483647)}) {
            if (n == 2147483647 && arg > 0 && arg < 4096) continue;      // (tens of millions of chunks to walk)
            check_chunks(n, arg);
        }
    {
        const genphi::RetainChunks a = genphi::retain_chunks(8191, 0), b = genphi::retain_chunks(8192, 0), c = genphi::retain_chunks(8193, 0),
                                   m = genphi::retain_chunks(1000000, 0), t = genphi::retain_chunks(2, 0), f = genphi::retain_chunks(1000000, 4096),
                                   w = genphi::retain_chunks(1000000, 20000), e = genphi::retain_chunks(16385, 16384);
        expect(a.chunks == 1 && a.chunk_labels == 8191 && a.bitmap_dwords == 256 && a.stride == 257 && a.lds_bytes == 65792, "default below the edge", 8191);
        expect(b.chunks == 1 && b.chunk_labels == 8192 && b.bitmap_dwords == 257 && b.stride == 257, "default at the edge", 8192);
        expect(c.chunks == 2 && c.chunk_labels == 8192 && c.lds_bytes == 65792, "default above the edge", 8193);
        expect(m.chunks == 123 && m.chunk_labels == 8192, "10^6 labels", 1000000);
        expect(t.chunks == 1 && t.chunk_labels == 2 && t.bitmap_dwords == 1 && t.stride == 1 && t.lds_bytes == 256, "two labels", 2);
        expect(f.chunks == 245 && f.chunk_labels == 4096 && f.bitmap_dwords == 129 && f.stride == 129 && f.lds_bytes == 33024, "forced 4096", 4096);
        expect(w.chunks == 62 && w.chunk_labels == 16384 && w.bitmap_dwords == 513 && w.stride == 513 && w.lds_bytes == 131328, "the widest chunk", 20000);
        expect(e.chunks == 2 && e.chunk_labels == 16384, "forced 16384", 16385);
    }
    // ---- the sizes and the panel rule on random plans ----
    long plans = 0, fits = 0, narrowed = 0, refused = 0;
    for (long k = 0; k < 20000; ++k) {
        genphi::IdentPlan pl;
        pl.n_live = 1 + below(k % 100 == 0 ? 3000000 : 5000);
        pl.n_pro = 1 + below(k % 7 == 0 ? 200000 : 300);
        pl.n_labels = 2 + below(2 * pl.n_live - 1);
        pl.planes = 1;
        while ((int64_t(1) << pl.planes) < pl.n_labels) ++pl.planes;
        pl.fa_row.resize(pl.n_live);
        pl.mo_row.resize(pl.n_live);
        pl.row_id.resize(pl.n_live);
        pl.pro_row.resize(pl.n_pro);
        pl.const_side.resize(pl.n_labels);
        const int64_t S = 1 + below(k % 3 == 0 ? (1 << 24) : 6000);
        const genphi::RetainSizes z = genphi::retain_sizes(pl, S);
        ++plans;
        expect(z.survived == static_cast<size_t>(4 * pl.n_labels) && z.both == z.survived && z.distinct == static_cast<size_t>(4 * S), "result bytes", k);
        expect(z.lists == static_cast<size_t>(4 * (2 * pl.n_live + pl.n_pro) + 8 * (pl.n_live + pl.n_labels)), "list bytes", k);
        const genphi::IdentSizes iz = genphi::ident_sizes(pl, S, false);
        expect(z.pair_rows == static_cast<size_t>(32 * pl.planes * pl.n_live) && z.pair_rows == iz.pair_rows && z.lists == iz.lists, "row bytes are ident's", k);
        expect(z.fixed() == z.survived + z.both + z.distinct + z.lists && z.panel(3) == 3 * z.pair_rows, "sums", k);
        expect(z.fixed() < iz.fixed() + 8 * static_cast<size_t>(pl.n_labels) + 4 * static_cast<size_t>(S) && z.panel(1) < iz.panel(1), "no counts, no gather", k);
        // the panel rule
        const int64_t total = (S + 127) / 128;
        const double pair_bytes = static_cast<double>(z.panel(1));
        const double room = static_cast<double>(below(4)) * pair_bytes * static_cast<double>(total) / 2.0 + static_cast<double>(below(1000)) - 300.0;
        for (int64_t arg : {int64_t(0), int64_t(128), int64_t(1000), S + 5}) {
            int64_t Pn = -7;
            const bool ok = genphi::drop_panel_fits(Pn, S, arg, room, pair_bytes);
            const int64_t asked = arg > 0 ? (total < (arg + 127) / 128 ? total : (arg + 127) / 128) : total;
            if (ok) {
                ++fits;
                expect(Pn >= 1 && Pn <= asked && pair_bytes * static_cast<double>(Pn) <= room, "a panel that fits", k);
                expect(arg == 0 || Pn == asked, "a forced panel is not narrowed", k);
                expect(arg != 0 || Pn == asked || pair_bytes * static_cast<double>(Pn + 1) > room, "the default is the widest that fits", k);
                narrowed += Pn < asked;
            } else {
                ++refused;
                expect(room < 0.0 || (arg == 0 ? (Pn < 1 || pair_bytes * static_cast<double>(Pn) > room) : pair_bytes * static_cast<double>(asked) > room), "a refusal has a reason", k);
            }
        }
    }
    std::printf("retain check: %ld chunk cases, %ld chunks walked, %ld borders with a halo, %ld plans, %ld panels fit, %ld narrowed, %ld refused; %ld violations\n",
                chunk_cases, chunks_walked, split_borders, plans, fits, narrowed, refused, violations);
    return violations ? 1 : 0;
}
