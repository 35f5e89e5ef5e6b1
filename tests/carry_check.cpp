// carry_check.cpp -- the host side of gen.simuCarriers (csrc/carry.h) as a stand-alone program: built by tests/test_carriers_host.py
// with g++, plain and under AddressSanitizer + UndefinedBehaviorSanitizer.  carry.h is header-only, and its functions read the sizes
// and the listed rows of a plan alone, so the plans here are lists of random lengths.  Checked: the chunk rule at n_labels = 1, 31, 32,
// 33, 255, 256, 257 and at the LDS ceiling (607, 608, 609), for the default and for forced widths, by walking every chunk; the two lists as sets of
// rows on random lists with repeats, against a restatement with std::set, and the overlap refusal; the columns and the limits at
// their edges; carry_sizes against the byte counts restated here.  Prints one summary line; exit status 1 on any violation.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <set>

#include "../genlib.jl_amd/csrc/carry.h"

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
void expect(bool ok, const char *what, long long at)
{
    if (ok) return;
    ++violations;
    std::fprintf(stderr, "VIOLATION at %lld: %s\n", at, what);
}

long chunk_cases = 0, chunks_walked = 0;

// One (n_labels, chunk_arg): the rule's numbers, and a walk over the chunks: they tile [0, n_labels) from multiples of the width, and
// every dword a lane addresses lies inside the 64 tables.
void check_chunks(int64_t n_labels, int64_t arg)
{
    const genphi::CarryChunks c = genphi::carry_chunks(n_labels, arg);
    const long long at = n_labels * 100000 + arg;
    ++chunk_cases;
    int64_t want = arg > 0 ? (arg + 31) / 32 * 32 : 608;
    if (want > 608) want = 608;
    if (want > n_labels) want = n_labels;
    expect(c.chunk_labels == want, "chunk width", at);
    expect(c.chunk_labels >= 1 && c.chunk_labels <= n_labels && c.chunk_labels <= genphi::CARRY_MAX_CHUNK, "chunk width range", at);
    expect(c.chunk_labels == n_labels || c.chunk_labels % 32 == 0, "a chunk narrower than the table is a multiple of 32", at);
    expect(c.chunks == (n_labels + c.chunk_labels - 1) / c.chunk_labels, "chunk count", at);
    expect(c.stride % 2 == 1 && c.stride >= c.chunk_labels && c.stride <= c.chunk_labels + 1, "odd stride", at);
    expect(c.lds_bytes == 256u * static_cast<size_t>(c.stride) && c.lds_bytes <= genphi::CARRY_LDS_BYTES, "LDS bytes", at);
    expect(63 * static_cast<int64_t>(c.stride) + c.chunk_labels - 1 < static_cast<int64_t>(c.lds_bytes / 4), "the last lane's last dword lies in the tables", at);
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
        expect(l0 == covered && l1 > l0 && l1 - l0 <= c.chunk_labels, "chunks tile the table", at);
        covered = l1;
        ++chunks_walked;
    }
    expect(covered == n_labels, "coverage", at);
}

}  // namespace

int main()
{
    // ---- the chunk rule ----
    for (int64_t n : {int64_t(1), int64_t(2), int64_t(31), int64_t(32), int64_t(33), int64_t(63), int64_t(64), int64_t(65), int64_t(255), int64_t(256), int64_t(257),
                      int64_t(607), int64_t(608), int64_t(609), int64_t(640), int64_t(14798), int64_t(1000000), int64_t(2147483647)})
        for (int64_t arg : {int64_t(0), int64_t(1), int64_t(31), int64_t(32), int64_t(33), int64_t(64), int64_t(128), int64_t(256), int64_t(257), int64_t(512),
                            int64_t(577), int64_t(608), int64_t(609), int64_t(640), int64_t(2147483647)}) {
            if (n == 2147483647 && arg > 0 && arg < 128) continue;       // (tens of millions of chunks to walk)
            check_chunks(n, arg);
        }
    {
        const genphi::CarryChunks one = genphi::carry_chunks(1, 0), a = genphi::carry_chunks(255, 0), b = genphi::carry_chunks(256, 0), c = genphi::carry_chunks(257, 256),
                                   d = genphi::carry_chunks(608, 0), g = genphi::carry_chunks(609, 0), m = genphi::carry_chunks(14798, 0),
                                   f = genphi::carry_chunks(257, 32), w = genphi::carry_chunks(14798, 100000), e = genphi::carry_chunks(609, 608),
                                   t = genphi::carry_chunks(33, 1), u = genphi::carry_chunks(31, 64);
        expect(one.chunks == 1 && one.chunk_labels == 1 && one.stride == 1 && one.lds_bytes == 256, "one label", 1);
        expect(a.chunks == 1 && a.chunk_labels == 255 && a.stride == 255 && a.lds_bytes == 65280, "255 labels", 255);
        expect(b.chunks == 1 && b.chunk_labels == 256 && b.stride == 257 && b.lds_bytes == 65792, "256 labels", 256);
        expect(c.chunks == 2 && c.chunk_labels == 256 && c.lds_bytes == 65792, "forced 256", 257);
        expect(d.chunks == 1 && d.chunk_labels == 608 && d.stride == 609 && d.lds_bytes == 155904, "default at the edge", 608);
        expect(g.chunks == 2 && g.chunk_labels == 608 && g.lds_bytes == 155904, "default above the edge", 609);
        expect(m.chunks == 25 && m.chunk_labels == 608, "14,798 labels", 14798);
        expect(f.chunks == 9 && f.chunk_labels == 32 && f.stride == 33 && f.lds_bytes == 8448, "forced 32", 32);
        expect(w.chunks == 25 && w.chunk_labels == 608 && w.stride == 609 && w.lds_bytes == 155904, "the widest chunk", 608);
        expect(e.chunks == 2 && e.chunk_labels == 608, "forced 608", 609);
        expect(t.chunks == 2 && t.chunk_labels == 32, "1 rounds up to 32", 33);
        expect(u.chunks == 1 && u.chunk_labels == 31 && u.stride == 31, "cut to the table", 31);
        // the ceiling: the next multiple of 32 does not fit
        expect(256u * static_cast<size_t>((genphi::CARRY_MAX_CHUNK + 32) | 1) > genphi::CARRY_LDS_BYTES && genphi::CARRY_MAX_CHUNK % 32 == 0, "CARRY_MAX_CHUNK is the largest", 0);
    }
    // ---- the columns and the limits ----
    expect(genphi::carry_columns(5, 0) == 6 && genphi::carry_columns(5, 3) == 4 && genphi::carry_columns(5, 5) == 6 && genphi::carry_columns(5, 9) == 6 &&
               genphi::carry_columns(1, 1) == 2 && genphi::carry_columns(32767, 0) == 32768,
           "columns", 0);
    expect(genphi::carry_limits(1, 2, 2).empty() && genphi::carry_limits(32767, 65534, 32768).empty(), "limits that hold", 0);
    expect(!genphi::carry_limits(0, 2, 1).empty() && !genphi::carry_limits(32768, 65536, 2).empty(), "no cases; too many cases", 0);
    expect(genphi::carry_limits(32767, 65535, 32768).empty() && !genphi::carry_limits(32767, 65536, 32768).empty(), "the cell limit at its edge", 0);
    expect(genphi::carry_limits(7, 2147483647, 1).empty() && !genphi::carry_limits(7, 1073741824, 2).empty() && genphi::carry_limits(7, 1073741823, 2).empty(),
           "the cell limit at two columns", 0);
    // ---- the lists and the sizes on random plans ----
    long plans = 0, overlaps = 0, repeats = 0;
    for (long k = 0; k < 20000; ++k) {
        genphi::IdentPlan pl;
        pl.n_live = 2 + below(k % 100 == 0 ? 300000 : 3000);
        const int64_t n_case_ids = 1 + below(k % 7 == 0 ? 5000 : 60), n_control_ids = k % 3 == 0 ? 0 : below(40);
        pl.n_pro = n_case_ids + n_control_ids;
        pl.n_labels = 2 + below(2 * pl.n_live - 1);
        pl.planes = 1;
        while ((int64_t(1) << pl.planes) < pl.n_labels) ++pl.planes;
        pl.fa_row.resize(pl.n_live);
        pl.mo_row.resize(pl.n_live);
        pl.row_id.resize(pl.n_live);
        for (int64_t r = 0; r < pl.n_live; ++r) pl.row_id[r] = 1000 + 3 * r;
        pl.const_side.resize(pl.n_labels);
        pl.pro_row.resize(pl.n_pro);
        // cases from the lower part of the rows, controls from the upper part; now and then one control is a case
        const int64_t cut = 1 + below(pl.n_live - 1);
        std::set<int32_t> cases, controls;
        for (int64_t i = 0; i < n_case_ids; ++i) cases.insert(pl.pro_row[i] = static_cast<int32_t>(below(cut)));
        const bool overlap = n_control_ids > 0 && k % 5 == 0;
        for (int64_t i = 0; i < n_control_ids; ++i)
            controls.insert(pl.pro_row[n_case_ids + i] = static_cast<int32_t>(overlap && i == n_control_ids / 2 ? pl.pro_row[below(n_case_ids)] : cut + below(pl.n_live - cut)));
        bool meets = false;
        for (int32_t r : controls) meets = meets || cases.count(r);
        genphi::CarryLists ls;
        int64_t both_id = -1;
        const bool refused = genphi::carry_lists(ls, pl, n_case_ids, both_id);
        ++plans;
        expect(refused == meets, "an overlap is refused, and nothing else", k);
        if (refused) {
            ++overlaps;
            expect(both_id >= 1000 && (both_id - 1000) % 3 == 0 && cases.count(static_cast<int32_t>((both_id - 1000) / 3)) && controls.count(static_cast<int32_t>((both_id - 1000) / 3)),
                   "the ID named stands in both lists", k);
            continue;
        }
        repeats += static_cast<int64_t>(cases.size()) < n_case_ids;
        expect(ls.n_cases == static_cast<int64_t>(cases.size()) && ls.n_controls == static_cast<int64_t>(controls.size()) &&
                   ls.rows.size() == cases.size() + controls.size(),
               "the distinct rows are counted", k);
        size_t at = 0;
        bool same = ls.rows.size() == cases.size() + controls.size();
        for (int32_t r : cases) same = same && ls.rows[at++] == r;      // (a std::set walks ascending)
        for (int32_t r : controls) same = same && ls.rows[at++] == r;
        expect(same, "cases ascending, then controls ascending", k);
        const int64_t max_count = below(3) == 0 ? 0 : 1 + below(2 * ls.n_cases);
        const int64_t W = genphi::carry_columns(ls.n_cases, max_count);
        expect(W == (max_count == 0 || max_count > ls.n_cases ? ls.n_cases : max_count) + 1, "columns", k);
        const genphi::CarrySizes z = genphi::carry_sizes(pl, ls, W);
        expect(z.excluded == static_cast<size_t>(4 * pl.n_labels) && z.carriers == static_cast<size_t>(4 * pl.n_labels * W) && z.homozygotes == z.carriers, "result bytes", k);
        expect(z.lists == static_cast<size_t>(4 * (2 * pl.n_live + pl.n_pro) + 8 * (pl.n_live + pl.n_labels) + 4 * (ls.n_cases + ls.n_controls)), "list bytes", k);
        const genphi::IdentSizes iz = genphi::ident_sizes(pl, 1000, false);
        expect(z.pair_rows == static_cast<size_t>(32 * pl.planes * pl.n_live) && z.pair_rows == iz.pair_rows, "row bytes are ident's", k);
        expect(z.fixed() == z.excluded + 2 * z.carriers + z.lists && z.panel(3) == 3 * z.pair_rows, "sums", k);
    }
    std::printf("carry check: %ld chunk cases, %ld chunks walked, %ld plans, %ld overlaps refused, %ld lists with repeats; %ld violations\n", chunk_cases,
                chunks_walked, plans, overlaps, repeats, violations);
    return violations ? 1 : 0;
}
