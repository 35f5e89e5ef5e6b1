// unique_check.cpp -- the host side of gen.simuUniqueness (csrc/unique.h) as a stand-alone program: built by
// tests/test_uniqueness_host.py with g++, plain and under AddressSanitizer + UndefinedBehaviorSanitizer.  unique.h is header-only, and
// its functions read the sizes and the listed rows of a plan alone, so the plans here are lists of random lengths.  Checked: the chunk
// rule at n_labels = 1, 2, 63, 64, 65 and at the LDS ceiling (1,215, 1,216, 1,217), for the default and for forced widths, by walking
// every chunk and every label's half of a dword; the two lists as sets of rows on random lists with repeats and overlaps, against a
// restatement with std::set; the columns and the limits at their edges; unique_sizes against the byte counts restated here.  Prints one
// summary line; exit status 1 on any violation.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <set>

#include "../genlib.jl_amd/csrc/unique.h"

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
// every half of a dword that a lane addresses lies inside the 64 tables and belongs to one label alone.
void check_chunks(int64_t n_labels, int64_t arg)
{
    const genphi::UniqueChunks c = genphi::unique_chunks(n_labels, arg);
    const long long at = n_labels * 100000 + arg;
    ++chunk_cases;
    int64_t want = arg > 0 ? (arg + 63) / 64 * 64 : genphi::UNIQUE_DEFAULT_CHUNK;
    if (want > 1216) want = 1216;
    if (want > n_labels) want = n_labels;
    expect(c.chunk_labels == want, "chunk width", at);
    expect(c.chunk_labels >= 1 && c.chunk_labels <= n_labels && c.chunk_labels <= genphi::UNIQUE_MAX_CHUNK, "chunk width range", at);
    expect(c.chunk_labels == n_labels || c.chunk_labels % 64 == 0, "a chunk narrower than the table is a multiple of 64", at);
    expect(c.chunks == (n_labels + c.chunk_labels - 1) / c.chunk_labels, "chunk count", at);
    const int64_t dwords = (c.chunk_labels + 1) / 2;
    expect(c.stride % 2 == 1 && c.stride >= dwords && c.stride <= dwords + 1, "odd stride", at);
    expect(c.lds_bytes == 256u * static_cast<size_t>(c.stride) && c.lds_bytes <= genphi::UNIQUE_LDS_BYTES && c.lds_bytes <= 163840, "LDS bytes", at);
    expect(63 * static_cast<int64_t>(c.stride) + ((c.chunk_labels - 1) >> 1) < static_cast<int64_t>(c.lds_bytes / 4), "the last lane's last dword lies in the tables", at);
    // 64 lanes at dword s * stride + d: 64 different banks modulo 32 within each half of the wave, and modulo 64 over the wave
    bool seen32[2][32] = {}, seen64[64] = {};
    bool clash = false;
    for (int s = 0; s < 64; ++s) {
        const int b32 = static_cast<int>((static_cast<int64_t>(s) * c.stride) % 32), b64 = static_cast<int>((static_cast<int64_t>(s) * c.stride) % 64);
        clash = clash || seen32[s / 32][b32] || seen64[b64];
        seen32[s / 32][b32] = seen64[b64] = true;
    }
    expect(!clash, "bank conflict", at);
    // label t of a chunk: half t & 1 of dword t >> 1; two labels never share a half
    if (c.chunk_labels <= 1216) {
        bool used[2 * 640] = {};
        bool twice = false;
        for (int64_t t = 0; t < c.chunk_labels; ++t) {
            const int64_t half = 2 * (t >> 1) + (t & 1);
            twice = twice || used[half] || (t >> 1) >= c.stride;
            used[half] = true;
        }
        expect(!twice, "one half of a dword per label", at);
    }
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
    for (int64_t n : {int64_t(1), int64_t(2), int64_t(3), int64_t(63), int64_t(64), int64_t(65), int64_t(127), int64_t(128), int64_t(129), int64_t(607), int64_t(608),
                      int64_t(609), int64_t(1215), int64_t(1216), int64_t(1217), int64_t(1280), int64_t(14798), int64_t(1000000), int64_t(2147483647)})
        for (int64_t arg : {int64_t(0), int64_t(1), int64_t(63), int64_t(64), int64_t(65), int64_t(128), int64_t(608), int64_t(609), int64_t(1153), int64_t(1216),
                            int64_t(1217), int64_t(1280), int64_t(5000), int64_t(2147483647)}) {
            if (n == 2147483647 && arg > 0 && arg <= 128) continue;      // (tens of millions of chunks to walk)
            check_chunks(n, arg);
        }
    {
        const genphi::UniqueChunks one = genphi::unique_chunks(1, 0), two = genphi::unique_chunks(2, 64), three = genphi::unique_chunks(3, 0),
                                    a = genphi::unique_chunks(63, 64), b = genphi::unique_chunks(64, 1), c = genphi::unique_chunks(65, 1), d = genphi::unique_chunks(65, 65),
                                    e = genphi::unique_chunks(1215, 1216), f = genphi::unique_chunks(1216, 5000), g = genphi::unique_chunks(1217, 1216),
                                    m = genphi::unique_chunks(14798, 1216), w = genphi::unique_chunks(14798, 608);
        expect(one.chunks == 1 && one.chunk_labels == 1 && one.stride == 1 && one.lds_bytes == 256, "one label", 1);
        expect(two.chunks == 1 && two.chunk_labels == 2 && two.stride == 1 && two.lds_bytes == 256, "two labels share a dword", 2);
        expect(three.chunks == 1 && three.chunk_labels == 3 && three.stride == 3, "three labels: two dwords, the last half unused", 3);
        expect(a.chunks == 1 && a.chunk_labels == 63 && a.stride == 33 && a.lds_bytes == 8448, "63 labels", 63);
        expect(b.chunks == 1 && b.chunk_labels == 64 && b.stride == 33, "1 rounds up to 64", 64);
        expect(c.chunks == 2 && c.chunk_labels == 64 && c.stride == 33, "65 labels in chunks of 64", 65);
        expect(d.chunks == 1 && d.chunk_labels == 65 && d.stride == 33, "65 rounds up to 128 and is cut to the table", 65);
        expect(e.chunks == 1 && e.chunk_labels == 1215 && e.stride == 609 && e.lds_bytes == 155904, "1,215 labels", 1215);
        expect(f.chunks == 1 && f.chunk_labels == 1216 && f.stride == 609 && f.lds_bytes == 155904, "5,000 is cut to 1,216", 1216);
        expect(g.chunks == 2 && g.chunk_labels == 1216, "1,217 labels", 1217);
        expect(m.chunks == 13 && m.chunk_labels == 1216 && w.chunks == 24 && w.chunk_labels == 640 && w.stride == 321 && w.lds_bytes == 82176, "14,798 labels; 608 rounds up to 640", 14798);
        // the ceiling: the next multiple of 64 does not fit, and the widest chunk is twice carry.h's
        expect(256u * static_cast<size_t>(((genphi::UNIQUE_MAX_CHUNK + 64) / 2) | 1) > genphi::UNIQUE_LDS_BYTES && genphi::UNIQUE_MAX_CHUNK % 64 == 0 &&
                   genphi::UNIQUE_MAX_CHUNK == 1216 && genphi::UNIQUE_MAX_CHUNK == 2 * genphi::CARRY_MAX_CHUNK,
               "UNIQUE_MAX_CHUNK is the largest", 0);
        expect(genphi::UNIQUE_DEFAULT_CHUNK % 64 == 0 && genphi::UNIQUE_DEFAULT_CHUNK >= 64 && genphi::UNIQUE_DEFAULT_CHUNK <= genphi::UNIQUE_MAX_CHUNK, "the default chunk", 0);
        // a 16-bit field never carries: the largest count fits, in either half
        expect(genphi::UNIQUE_MAX_POP == 0xFFFF && (static_cast<uint64_t>(genphi::UNIQUE_MAX_POP) << 16 | genphi::UNIQUE_MAX_POP) == 0xFFFFFFFFull, "the fields at their ends", 0);
    }
    // ---- the columns and the limits ----
    expect(genphi::unique_columns(5, 0) == 5 && genphi::unique_columns(5, 3) == 3 && genphi::unique_columns(5, 5) == 5 && genphi::unique_columns(5, 9) == 5 &&
               genphi::unique_columns(1, 1) == 1 && genphi::unique_columns(65535, 0) == 65535,
           "columns", 0);
    expect(genphi::unique_limits(1, 1, 1).empty() && genphi::unique_limits(1, 65535, 65535).empty() && genphi::unique_limits(32768, 65535, 65535).empty(), "limits that hold", 0);
    expect(!genphi::unique_limits(0, 2, 2).empty() && genphi::unique_limits(0, 2, 2) == "no probands", "no probands", 0);
    expect(!genphi::unique_limits(1, 65536, 8).empty() && genphi::unique_limits(1, 65536, 8).find("65,535") != std::string::npos, "n_pop = 65,536 is refused", 0);
    expect(genphi::unique_limits(65535, 65535, 8).empty() && !genphi::unique_limits(65536, 65536, 8).empty(), "n_pop at its edge with every member a proband", 0);
    // 2^31 - 1 is prime: n x K meets it exactly only with one row or one column (the function takes any K; create never passes one above
    // n_pop).  At 65,535 columns 32,768 rows are 2^31 - 32,768 cells and hold, 32,769 rows are 2^31 + 32,767 and do not
    expect(genphi::unique_limits(32768, 65535, 65535).empty() && !genphi::unique_limits(32769, 65535, 65535).empty(), "the cell limit at 65,535 columns", 0);
    expect(genphi::unique_limits(1, 65535, 2147483647).empty() && genphi::unique_limits(2147483647, 65535, 1).empty() && !genphi::unique_limits(2, 65535, 1073741824).empty() &&
               genphi::unique_limits(2, 65535, 1073741823).empty() && !genphi::unique_limits(1073741824, 65535, 2).empty(),
           "the cell limit at 2^31 - 1 and 2^31", 0);
    expect(genphi::unique_limits(32769, 65535, 65535).find("pass a smaller maxShare") != std::string::npos, "the cell limit's advice", 0);
    // ---- the lists and the sizes on random plans ----
    long plans = 0, overlaps = 0, repeats = 0;
    for (long k = 0; k < 20000; ++k) {
        genphi::IdentPlan pl;
        pl.n_live = 2 + below(k % 100 == 0 ? 300000 : 3000);
        const int64_t n_pro_ids = 1 + below(k % 7 == 0 ? 5000 : 60), n_other_ids = k % 3 == 0 ? 0 : below(40);
        pl.n_pro = n_pro_ids + n_other_ids;
        pl.n_labels = 2 + below(2 * pl.n_live - 1);
        pl.planes = 1;
        while ((int64_t(1) << pl.planes) < pl.n_labels) ++pl.planes;
        pl.fa_row.resize(pl.n_live);
        pl.mo_row.resize(pl.n_live);
        pl.row_id.resize(pl.n_live);
        for (int64_t r = 0; r < pl.n_live; ++r) pl.row_id[r] = 1000 + 3 * r;
        pl.const_side.resize(pl.n_labels);
        pl.pro_row.resize(pl.n_pro);
        // probands from the lower part of the rows, others from the upper part; in every fifth plan some others are probands
        const int64_t cut = 1 + below(pl.n_live - 1);
        std::set<int32_t> pro, others;
        for (int64_t i = 0; i < n_pro_ids; ++i) pro.insert(pl.pro_row[i] = static_cast<int32_t>(below(cut)));
        const bool overlap = n_other_ids > 0 && k % 5 == 0;
        bool met = false;
        for (int64_t i = 0; i < n_other_ids; ++i) {
            const bool both = overlap && i % 2 == 0;
            const int32_t r = pl.pro_row[n_pro_ids + i] = static_cast<int32_t>(both ? pl.pro_row[below(n_pro_ids)] : cut + below(pl.n_live - cut));
            if (both) met = true;
            else others.insert(r);
        }
        overlaps += met;
        genphi::UniqueLists ls;
        genphi::unique_lists(ls, pl, n_pro_ids);
        ++plans;
        repeats += static_cast<int64_t>(pro.size()) < n_pro_ids;
        expect(ls.n_pro == static_cast<int64_t>(pro.size()) && ls.n_others == static_cast<int64_t>(others.size()) && ls.rows.size() == pro.size() + others.size() &&
                   ls.n_pop() == ls.n_pro + ls.n_others,
               "the distinct rows are counted, an other that is a proband once, as a proband", k);
        size_t at = 0;
        bool same = ls.rows.size() == pro.size() + others.size();
        for (int32_t r : pro) same = same && ls.rows[at++] == r;         // (a std::set walks ascending)
        for (int32_t r : others) same = same && ls.rows[at++] == r;
        expect(same, "probands ascending, then the others ascending", k);
        const int64_t max_share = below(3) == 0 ? 0 : 1 + below(2 * ls.n_pop());
        const int64_t K = genphi::unique_columns(ls.n_pop(), max_share);
        expect(K == (max_share == 0 || max_share > ls.n_pop() ? ls.n_pop() : max_share) && K >= 1, "columns", k);
        const genphi::UniqueSizes z = genphi::unique_sizes(pl, ls, K);
        expect(z.alleles == static_cast<size_t>(4 * ls.n_pro * K) && z.autozygous == z.alleles, "result bytes", k);
        expect(z.lists == static_cast<size_t>(4 * (2 * pl.n_live + pl.n_pro) + 8 * (pl.n_live + pl.n_labels) + 4 * ls.n_pop()), "list bytes", k);
        const genphi::IdentSizes iz = genphi::ident_sizes(pl, 1000, false);
        expect(z.pair_rows == static_cast<size_t>(32 * pl.planes * pl.n_live) && z.pair_rows == iz.pair_rows, "row bytes are ident's", k);
        expect(z.fixed() == 2 * z.alleles + z.lists && z.panel(3) == 3 * z.pair_rows, "sums", k);
    }
    std::printf("unique check: %ld chunk cases, %ld chunks walked, %ld plans, %ld overlaps folded, %ld lists with repeats; %ld violations\n", chunk_cases,
                chunks_walked, plans, overlaps, repeats, violations);
    return violations ? 1 : 0;
}
