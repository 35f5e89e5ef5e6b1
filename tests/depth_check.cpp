// The word arithmetic of gen.depths (csrc/depth_word.h) on the host schedule it runs on (csrc/ancestor_sweep.cpp: plan_sweep with the
// options of genphi_depth_create), checked without a GPU.  Built and run by tests/test_depth_host.py, plain and under AddressSanitizer +
// UndefinedBehaviorSanitizer.  Links ancestor_sweep.cpp and planner.cpp directly -- no HIP, no oracle.
//
//   1. Random pedigrees of at most 60 individuals from a generator of its own (SplitMix64, fixed seeds): parents from a window of earlier
//      ranks, one-parent members, founders anywhere; proband lists with leaves, members with children, listed ancestors and repeats; ancestor
//      lists with founders, members with parents, probands, unrelated members and repeats.  The items of the schedule are interpreted with one
//      row of DepthWord per slot (depth_step, depth_onehot, the copy rule), and every result entry is unpacked and compared with a recursive
//      enumeration of every ascending path that knows neither cuts nor slots nor words.
//   2. On every row written, slot or result: max <= n_steps (the bound the packing rests on) and P < 2^48.
//   3. The sib-mating ladder: two founders, then 47 generations of two full sibs each.  P = 2^46 per founder and S = 47 * 2^46: the packed
//      fields at their limit (47 steps).  A variant whose last member has one generation-skipping mate, so that min < mean < max.  Far too
//      many paths to enumerate: compared with the closed forms and with a memoised recursion on unpacked fields.
// Prints one summary line; exit status 1 after any violation.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../genlib.jl_amd/csrc/ancestor_sweep.h"
#include "../genlib.jl_amd/csrc/depth_word.h"
#include "../include/genphi.h"

using genphi::DepthWord;
using genphi::SweepItem;
using genphi::SweepSchedule;

namespace {

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed) {}
    uint64_t next()
    {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    int below(int n) { return static_cast<int>(next() % static_cast<uint64_t>(n)); }          // n >= 1
    bool chance(int permille) { return below(1000) < permille; }
};

// rank order (parents first); fa / mo are ranks, -1 = unknown; the ID of rank i is i + 1
struct Ped {
    std::vector<int32_t> fa, mo;
    int n() const { return static_cast<int>(fa.size()); }
};

// what the result says about one pair, unpacked
struct Stat {
    uint64_t paths = 0;
    int64_t sum = 0;
    int lo = -1, hi = -1;
    bool operator==(const Stat &o) const { return paths == o.paths && sum == o.sum && lo == o.lo && hi == o.hi; }
};

struct Counters {
    long pedigrees = 0, schedules = 0, rows = 0, entries = 0, copy_items = 0, one_parent = 0, pro_with_children = 0, pro_is_anc = 0, dup_pro = 0,
         dup_anc = 0, unrelated = 0, ladders = 0, violations = 0;
    uint64_t max_paths = 0;
    int max_far = 0;
} g;

std::string g_where;

bool fail(const char *what, long a = -1, long b = -1)
{
    if (g.violations < 20) std::fprintf(stderr, "VIOLATION %s: %s (%ld, %ld)\n", g_where.c_str(), what, a, b);
    ++g.violations;
    return false;
}

#define REQUIRE(cond, ...) do { if (!(cond)) return fail(__VA_ARGS__); } while (0)

Stat unpack(const DepthWord &v)
{
    Stat s;
    s.paths = genphi::depth_paths(v);
    s.sum = v.s;
    s.lo = genphi::depth_min_of(genphi::depth_close(v));
    s.hi = genphi::depth_max_of(genphi::depth_far(v));
    return s;
}

// every ascending path of x, one call per path: at[y] collects the paths that end at y
void enumerate(const Ped &p, int x, int length, std::vector<Stat> &at)
{
    Stat &s = at[x];
    ++s.paths;
    s.sum += length;
    s.lo = s.lo < 0 ? length : std::min(s.lo, length);
    s.hi = std::max(s.hi, length);
    if (p.fa[x] >= 0) enumerate(p, p.fa[x], length + 1, at);
    if (p.mo[x] >= 0) enumerate(p, p.mo[x], length + 1, at);
}

// the recursion on unpacked fields, top-down and memoised, one ancestor at a time (for pedigrees with too many paths to enumerate)
Stat recurse(const Ped &p, int x, int anc, std::vector<Stat> &memo, std::vector<char> &done)
{
    if (done[x]) return memo[x];
    Stat s;
    if (x == anc) {
        s.paths = 1; s.sum = 0; s.lo = 0; s.hi = 0;
    } else {
        for (int q : {p.fa[x], p.mo[x]}) {
            if (q < 0) continue;
            const Stat u = recurse(p, q, anc, memo, done);
            if (!u.paths) continue;
            s.lo = s.lo < 0 ? u.lo + 1 : std::min(s.lo, u.lo + 1);
            s.hi = std::max(s.hi, u.hi + 1);
            s.paths += u.paths;
            s.sum += u.sum + static_cast<int64_t>(u.paths);
        }
    }
    done[x] = 1;
    return memo[x] = s;
}

// plan_sweep with the options of genphi_depth_create, the items interpreted in depth_word.h's arithmetic: the result rows (pre-fill: the zero
// element, which unpacks to 0, -1, -1)
bool sweep(const Ped &p, const std::vector<int32_t> &pro, const std::vector<int32_t> &anc, std::vector<std::vector<DepthWord>> &res, int &n_steps)
{
    const int n = p.n();
    std::vector<int64_t> id(n), fa(n), mo(n), pro_ids, anc_ids;
    for (int i = 0; i < n; ++i) { id[i] = i + 1; fa[i] = p.fa[i] + 1; mo[i] = p.mo[i] + 1; }
    for (int32_t x : pro) pro_ids.push_back(x + 1);
    for (int32_t x : anc) anc_ids.push_back(x + 1);
    genphi::SweepOptions opt;
    opt.emit = genphi::Emit::EveryProband;
    opt.first_onehot_only = false;
    opt.mark_copies = true;
    SweepSchedule h;
    std::string err;
    const int rc = genphi::plan_sweep(h, n, id.data(), fa.data(), mo.data(), static_cast<int64_t>(pro.size()), pro_ids.data(),
                                      static_cast<int64_t>(anc.size()), anc_ids.data(), opt, err);
    REQUIRE(rc == GENPHI_OK, "plan_sweep failed", rc);
    ++g.schedules;
    n_steps = h.n_steps;
    const int W = static_cast<int>(anc.size());
    const DepthWord none{0, 0};
    res.assign(pro.size(), std::vector<DepthWord>(W, none));
    std::vector<std::vector<DepthWord>> slot(static_cast<size_t>(h.peak_slots), std::vector<DepthWord>(W, none));
    const int n_lists = static_cast<int>(h.list_to_result.size());
    for (int k = 0; k < n_lists; ++k) {
        const bool to_res = h.list_to_result[k] != 0;
        for (int64_t i = h.list_begin[k]; i < h.list_begin[k + 1] - 1; ++i) {
            const SweepItem &it = h.items[i];
            REQUIRE(it.a >= -1 && it.a < h.peak_slots && it.b >= -2 && it.b < h.peak_slots, "a source slot out of range", it.a, it.b);
            REQUIRE(it.dst >= 0 && it.dst < (to_res ? static_cast<int64_t>(pro.size()) : h.peak_slots), "a destination out of range", it.dst);
            const bool copy = it.b == -2;
            if (copy) ++g.copy_items;
            std::vector<DepthWord> row(W);
            for (int j = 0; j < W; ++j) row[j] = genphi::depth_step(it.a >= 0 ? slot[it.a][j] : none, it.b >= 0 ? slot[it.b][j] : none, copy ? 0u : 1u);
            for (int32_t q = it.oh; q < h.items[i + 1].oh; ++q) row[h.oh_cols[q]] = genphi::depth_onehot();
            for (int j = 0; j < W; ++j) {
                // the bounds the packing rests on, on every row written
                const int far = genphi::depth_max_of(genphi::depth_far(row[j]));
                REQUIRE(far <= h.n_steps, "max exceeds the steps of the sweep", far, h.n_steps);
                REQUIRE(genphi::depth_paths(row[j]) < (uint64_t(1) << 48) && (row[j].w & genphi::kDepthPathMask) == genphi::depth_paths(row[j]), "P >= 2^48");
                REQUIRE(genphi::depth_paths(row[j]) <= (uint64_t(1) << std::max(far, 0)), "P exceeds 2^max (Kraft)", far);
                REQUIRE((genphi::depth_paths(row[j]) == 0) == (row[j].w == 0 && row[j].s == 0), "a row without paths that is not the zero element");
                g.max_paths = std::max(g.max_paths, static_cast<uint64_t>(genphi::depth_paths(row[j])));
                g.max_far = std::max(g.max_far, far);
            }
            ++g.rows;
            (to_res ? res[it.dst] : slot[it.dst]) = row;
        }
    }
    return true;
}

bool check_random(const Ped &p, const std::vector<int32_t> &pro, const std::vector<int32_t> &anc)
{
    std::vector<std::vector<DepthWord>> res;
    int n_steps = 0;
    if (!sweep(p, pro, anc, res, n_steps)) return false;
    REQUIRE(n_steps <= GENPHI_DEPTH_MAX_STEPS, "the generator left its depth", n_steps);
    std::vector<std::vector<Stat>> memo(p.n());
    for (size_t i = 0; i < pro.size(); ++i) {
        std::vector<Stat> &at = memo[pro[i]];
        if (at.empty()) {
            at.assign(p.n(), Stat());
            enumerate(p, pro[i], 0, at);
        }
        for (size_t j = 0; j < anc.size(); ++j) {
            const Stat got = unpack(res[i][j]);
            REQUIRE(got == at[anc[j]], "a result entry differs from the enumeration", static_cast<long>(i), static_cast<long>(j));
            const double mean = genphi::depth_mean_of(got.paths, got.sum);
            REQUIRE(got.paths ? mean == static_cast<double>(got.sum) / static_cast<double>(got.paths) && mean >= got.lo && mean <= got.hi : std::isnan(mean),
                    "the mean", static_cast<long>(i), static_cast<long>(j));
            if (!got.paths) ++g.unrelated;
            ++g.entries;
        }
    }
    return true;
}

// generation g (1 .. generations) = ranks 2g - 2, 2g - 1, two full sibs whose parents are the two sibs of generation g - 1; skip: the mother of
// the last member comes from generation g - 2 instead
Ped ladder(int generations, bool skip)
{
    Ped p;
    p.fa.assign(2 * generations, -1);
    p.mo.assign(2 * generations, -1);
    for (int gnr = 2; gnr <= generations; ++gnr)
        for (int k = 0; k < 2; ++k) {
            p.fa[2 * gnr - 2 + k] = 2 * gnr - 4;
            p.mo[2 * gnr - 2 + k] = 2 * gnr - 3;
        }
    if (skip) p.mo[2 * generations - 1] = 2 * generations - 5;
    return p;
}

bool check_ladder(bool skip)
{
    const int G = GENPHI_DEPTH_MAX_STEPS + 1;                 // 48 generations: 47 steps, 96 individuals
    const Ped p = ladder(G, skip);
    const int last = 2 * G - 1;
    const std::vector<int32_t> pro = {last, last - 1, last, 2 * G - 4}, anc = {0, 1, 0, 2 * G - 4, 2 * G - 6, last};
    std::vector<std::vector<DepthWord>> res;
    int n_steps = 0;
    g_where = skip ? "the ladder with a generation-skipping mate" : "the sib-mating ladder";
    if (!sweep(p, pro, anc, res, n_steps)) return false;
    REQUIRE(n_steps == GENPHI_DEPTH_MAX_STEPS, "the ladder has other than 47 steps", n_steps);
    for (size_t j = 0; j < anc.size(); ++j) {
        std::vector<Stat> memo(p.n());
        std::vector<char> done(p.n(), 0);
        for (size_t i = 0; i < pro.size(); ++i) {
            const Stat want = recurse(p, pro[i], anc[j], memo, done), got = unpack(res[i][j]);
            REQUIRE(got == want, "a ladder entry differs from the unpacked recursion", static_cast<long>(i), static_cast<long>(j));
            ++g.entries;
        }
    }
    // the closed forms, last member x founders
    const uint64_t one = 1;
    for (size_t j = 0; j < 2; ++j) {
        const Stat got = unpack(res[0][j]);
        const double mean = genphi::depth_mean_of(got.paths, got.sum);
        if (!skip) {
            REQUIRE(got.paths == one << 46 && got.sum == static_cast<int64_t>(47 * (one << 46)) && got.lo == 47 && got.hi == 47 && mean == 47.0,
                    "the ladder's closed form");
        } else {
            // the father (generation 47): 2^45 paths of 46 meioses; the mother (generation 46): 2^44 paths of 45
            REQUIRE(got.paths == 3 * (one << 44) && got.sum == static_cast<int64_t>(47 * (one << 45) + 46 * (one << 44)) && got.lo == 46 && got.hi == 47,
                    "the skipping ladder's closed form");
            REQUIRE(mean > got.lo && mean < got.hi && mean == (47.0 * 2 + 46.0) / 3.0, "min < mean < max on the skipping ladder");
        }
    }
    const Stat sib = unpack(res[1][0]);                      // the other member of the last generation: the plain ladder either way
    REQUIRE(sib.paths == one << 46 && sib.lo == 47 && sib.hi == 47, "the last member's sib");
    ++g.ladders;
    return true;
}

}  // namespace

int main()
{
    const int kPedigrees = 2400;
    for (int c = 0; c < kPedigrees; ++c) {
        Rng r(20261019ull * 1000 + static_cast<uint64_t>(c));
        static const int sizes[] = {1, 2, 3, 5, 9, 17, 30, 48};
        const int n = sizes[r.below(8)] + r.below(13);                    // at most 60
        const int back = 2 + r.below(n);
        static const int founder_pm[] = {20, 100, 300}, one_pm[] = {0, 80, 350};
        const int fpm = founder_pm[r.below(3)], opm = one_pm[r.below(3)];
        Ped p;
        p.fa.assign(n, -1);
        p.mo.assign(n, -1);
        // paths[x]: the ascending paths of x (every end point), kept small enough to enumerate; depth[x]: its longest ascent
        std::vector<uint64_t> paths(n, 1);
        std::vector<int> depth(n, 0);
        std::vector<char> has_child(n, 0);
        for (int i = 1; i < n; ++i) {
            if (r.chance(fpm)) continue;
            const int lo = std::max(0, i - back);
            int f = lo + r.below(i - lo), m = lo + r.below(i - lo);
            if (r.chance(opm)) { if (r.chance(500)) f = -1; else m = -1; }
            const uint64_t np = 1 + (f >= 0 ? paths[f] : 0) + (m >= 0 ? paths[m] : 0);
            const int nd = 1 + std::max(f >= 0 ? depth[f] : -1, m >= 0 ? depth[m] : -1);
            if (np > 20000 || nd > GENPHI_DEPTH_MAX_STEPS) continue;      // a founder instead
            p.fa[i] = f; p.mo[i] = m; paths[i] = np; depth[i] = nd;
            if ((f < 0) != (m < 0)) ++g.one_parent;
            if (f >= 0) has_child[f] = 1;
            if (m >= 0) has_child[m] = 1;
        }
        ++g.pedigrees;
        for (int rep = 0; rep < 2; ++rep) {
            std::vector<int32_t> pro, anc;
            const int np = 1 + r.below(std::min(n, 12)), na = 1 + r.below(std::min(n, 20));
            for (int q = 0; q < np; ++q) pro.push_back(r.below(n));
            for (int q = 0; q < na; ++q) anc.push_back(r.chance(500) ? r.below(std::max(n / 3, 1)) : r.below(n));
            if (r.chance(500)) { anc.push_back(pro[r.below(static_cast<int>(pro.size()))]); }                  // a proband that is a listed ancestor
            if (r.chance(400)) { pro.push_back(pro[r.below(static_cast<int>(pro.size()))]); }                  // duplicated probands
            if (r.chance(400)) { anc.push_back(anc[r.below(static_cast<int>(anc.size()))]); }                  // duplicated ancestors
            std::vector<int32_t> sp = pro, sa = anc;
            std::sort(sp.begin(), sp.end());
            std::sort(sa.begin(), sa.end());
            if (std::adjacent_find(sp.begin(), sp.end()) != sp.end()) ++g.dup_pro;
            if (std::adjacent_find(sa.begin(), sa.end()) != sa.end()) ++g.dup_anc;
            for (int32_t x : pro) {
                if (has_child[x]) ++g.pro_with_children;
                if (std::binary_search(sa.begin(), sa.end(), x)) ++g.pro_is_anc;
            }
            g_where = "pedigree " + std::to_string(c) + " (n = " + std::to_string(n) + "), lists " + std::to_string(rep);
            check_random(p, pro, anc);
        }
    }
    check_ladder(false);
    check_ladder(true);
    if (!g.copy_items || !g.one_parent || !g.pro_with_children || !g.pro_is_anc || !g.dup_pro || !g.dup_anc || !g.unrelated)
        fail("the random cases did not reach every edge");
    std::printf("depth check: %ld pedigrees, %ld schedules, %ld rows (%ld copy items), %ld entries compared; %ld one-parent members, %ld probands with "
                "children, %ld probands that are listed ancestors, %ld lists with duplicated probands, %ld with duplicated ancestors, %ld pairs without "
                "a path; largest P %llu, longest ascent %d; %ld ladders of 47 steps; %ld violations\n",
                g.pedigrees, g.schedules, g.rows, g.copy_items, g.entries, g.one_parent, g.pro_with_children, g.pro_is_anc, g.dup_pro, g.dup_anc,
                g.unrelated, static_cast<unsigned long long>(g.max_paths), g.max_far, g.ladders, g.violations);
    return g.violations ? 1 : 0;
}
