// The host schedule of the ancestor sweeps (csrc/ancestor_sweep.cpp: plan_sweep), the one piece gen.gc, gen.occ, gen.rec, gen.meioses and
// gen.completeness all trust, checked without a GPU.  Built and run by tests/test_sweep_schedule.py, plain and under AddressSanitizer +
// UndefinedBehaviorSanitizer.  Links ancestor_sweep.cpp and planner.cpp directly -- no HIP, no oracle.
//
// Random pedigrees from a generator of its own (SplitMix64, fixed seeds): parents from several generations back, one-parent members,
// selfing, late founders; IDs dense (the direct table of Ranks), dense with holes in another order than the ranks, and sparse / negative
// (its hash map); proband lists with members of every depth, repeats, every individual, founders only, nobody, unknown IDs; ancestor lists
// with founders, non-founders, repeats, probands, unrelated individuals, everybody, nobody, an unknown ID.  For each of the five option
// sets of the callers (gc.hip, occ.hip, dist.hip, completeness.hip) plan_sweep is called and
//   1. the schedule is checked as a structure: lists, sentinels, one-hot offsets, slot bounds, no destination among the sources of its own
//      list, no destination twice, every source written by an earlier list and still owned by the member the item needs (the items of a
//      list are matched against the members that are new in that cut, found here by a walk of parent steps from the probands), peak_slots;
//   2. the items are interpreted with one row per slot in the arithmetic of that caller (Float64 halves, wrap-around sums, OR,
//      saturating closeness with the copy rule, shifted counts with the copy rule), and every result row (rec: every row of pro_slots) is
//      compared entry for entry with a memoised top-down recursion over the pedigree that knows neither cuts nor slots.
// Prints one summary line; exit status 1 after any violation.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../genlib.jl_amd/csrc/ancestor_sweep.h"
#include "../include/genphi.h"

using genphi::Emit;
using genphi::SweepItem;
using genphi::SweepOptions;
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
    template <class T> void shuffle(std::vector<T> &v)
    {
        for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[static_cast<size_t>(below(static_cast<int>(i)))]);
    }
};

// A pedigree in rank order (parents first); fa / mo are ranks (-1 = unknown), id the labels (never 0), hole an ID nobody carries.
struct Ped {
    std::vector<int32_t> fa, mo;
    std::vector<int64_t> id;
    std::vector<char> has_child;
    int64_t hole = 0;
    int n() const { return static_cast<int>(fa.size()); }
};

enum { kIdsDense = 0, kIdsHoles = 1, kIdsSparse = 2 };

void label(Ped &p, int mode, Rng &r)
{
    const int n = p.n();
    p.id.resize(n);
    if (mode == kIdsDense) {
        for (int i = 0; i < n; ++i) p.id[i] = i + 1;
        p.hole = r.chance(500) ? n + 1 + r.below(5000) : -1 - r.below(50);          // past the direct table, or negative
    } else if (mode == kIdsHoles) {
        std::vector<int64_t> perm(n);
        for (int i = 0; i < n; ++i) perm[i] = i;
        r.shuffle(perm);
        for (int i = 0; i < n; ++i) p.id[i] = 2 * perm[i] + 1;                       // odd labels < 2 n: still the direct table
        p.hole = 2 * (1 + r.below(std::max(n - 1, 1)));                              // an even label inside the table
    } else {
        std::set<int64_t> used{0};
        for (int i = 0; i < n; ++i) {
            int64_t v;
            do v = static_cast<int64_t>(r.next() >> 20) - (int64_t(1) << 43); while (used.count(v));
            used.insert(v);
            p.id[i] = v;
        }
        do p.hole = static_cast<int64_t>(r.next() >> 20) - (int64_t(1) << 43); while (used.count(p.hole));
    }
}

void finish(Ped &p)
{
    p.has_child.assign(p.n(), 0);
    for (int i = 0; i < p.n(); ++i) {
        if (p.fa[i] >= 0) p.has_child[p.fa[i]] = 1;
        if (p.mo[i] >= 0) p.has_child[p.mo[i]] = 1;
    }
}

// window: both parents among the `back` ranks before the child (overlapping generations of any reach);
// layered: generations `width` wide, a parent from the generation before or, with skip_pm, from up to four generations back
Ped random_ped(Rng &r, int n, bool layered, int back_or_width, int founder_pm, int one_pm, int self_pm, int skip_pm)
{
    Ped p;
    p.fa.assign(n, -1);
    p.mo.assign(n, -1);
    for (int i = 1; i < n; ++i) {
        if (r.chance(founder_pm)) continue;
        int f, m;
        if (!layered) {
            const int lo = std::max(0, i - back_or_width);
            f = lo + r.below(i - lo);
            m = lo + r.below(i - lo);
        } else {
            const int g = i / back_or_width;
            if (g == 0) continue;
            auto pick = [&]() {
                const int up = r.chance(skip_pm) ? std::min(g, 2 + r.below(3)) : 1;
                return (g - up) * back_or_width + r.below(back_or_width);
            };
            f = pick();
            m = pick();
        }
        if (r.chance(self_pm)) m = f;
        if (r.chance(one_pm)) { if (r.chance(500)) f = -1; else m = -1; }
        p.fa[i] = f;
        p.mo[i] = m;
    }
    finish(p);
    return p;
}

struct OptSet {
    const char *name;
    SweepOptions o;
    int arith;
};
enum { kGC = 0, kOcc, kRec, kDist, kComp, kFamilies };

// the options of the five callers, as gc.hip (genphi_gc_create), occ.hip (create_impl), dist.hip (genphi_dist_create) and completeness.hip
// (genphi_comp_create) set them
std::vector<OptSet> caller_options()
{
    std::vector<OptSet> v(kFamilies);
    v[kGC] = {"gc", SweepOptions(), kGC};
    v[kGC].o.emit = Emit::LeafFirst;
    v[kOcc] = {"occ", SweepOptions(), kOcc};
    v[kOcc].o.emit = Emit::EveryProband;
    v[kOcc].o.first_onehot_only = true;
    v[kRec] = {"rec", SweepOptions(), kRec};
    v[kRec].o.emit = Emit::None;
    v[kRec].o.drop_unknown_pro = true;
    v[kDist] = {"meioses", SweepOptions(), kDist};
    v[kDist].o.emit = Emit::EveryProband;
    v[kDist].o.mark_copies = true;
    v[kComp] = {"completeness", SweepOptions(), kComp};
    v[kComp].o.emit = Emit::EveryProband;
    v[kComp].o.mark_copies = true;
    v[kComp].o.every_member = true;
    return v;
}

struct Counters {
    long schedules = 0, items = 0, lists = 0, entries = 0, violations = 0;
    long founders_only[kFamilies] = {}, copy_items[kFamilies] = {}, empty_pro = 0, empty_anc_every_member = 0;
    long unknown_pro_error = 0, unknown_pro_dropped = 0, unknown_anc_error = 0, direct_ids = 0, hashed_ids = 0, reused_slots = 0;
} g;

std::string g_where;

bool fail(const char *what, long a = -1, long b = -1)
{
    if (g.violations < 20) std::fprintf(stderr, "VIOLATION %s: %s (%ld, %ld)\n", g_where.c_str(), what, a, b);
    ++g.violations;
    return false;
}

#define REQUIRE(cond, ...) do { if (!(cond)) return fail(__VA_ARGS__); } while (0)

// one row of W entries per slot / result row / individual, as unsigned 64-bit patterns (Float64 through its bits is not needed: gc keeps
// doubles of its own)
using Row = std::vector<uint64_t>;

// ---- the top-down recursions: row(x) from row(father), row(mother), memoised; no cuts, no slots ----------------------------------

struct TopDown {
    const Ped &p;
    int family, W;
    std::vector<std::vector<int32_t>> cols_of;      // per rank: the columns that carry its one-hot (occ: the first one only)
    std::vector<Row> memo_u;
    std::vector<std::vector<double>> memo_d;
    std::vector<char> done;
    TopDown(const Ped &ped, int fam, int width, const std::vector<int32_t> &anc_rank) : p(ped), family(fam), W(width)
    {
        cols_of.resize(p.n());
        for (size_t j = 0; j < anc_rank.size(); ++j)
            if (family != kOcc || cols_of[anc_rank[j]].empty()) cols_of[anc_rank[j]].push_back(static_cast<int32_t>(j));
        memo_u.resize(p.n());
        memo_d.resize(p.n());
        done.assign(p.n(), 0);
    }
    void need(int x)
    {
        if (done[x]) return;
        const int f = p.fa[x], m = p.mo[x];
        if (f >= 0) need(f);
        if (m >= 0) need(m);
        if (family == kGC) {
            std::vector<double> v(W, 0.0);
            for (int j = 0; j < W; ++j) v[j] = 0.5 * ((f >= 0 ? memo_d[f][j] : 0.0) + (m >= 0 ? memo_d[m][j] : 0.0));
            for (int32_t j : cols_of[x]) v[j] = 1.0;
            memo_d[x] = v;
        } else {
            Row v(W, 0);
            for (int j = 0; j < W; ++j) {
                const uint64_t a = f >= 0 ? memo_u[f][j] : 0, b = m >= 0 ? memo_u[m][j] : 0;
                switch (family) {
                case kOcc: v[j] = a + b; break;                                           // modulo 2^64
                case kRec: v[j] = a | b; break;
                case kDist: {                                                              // meioses + 1, 0 = no ascent
                    const uint64_t best = a && b ? std::min(a, b) : (a ? a : b);
                    v[j] = best ? best + 1 : 0;
                } break;
                default: {                                                                 // completeness: paths of exactly j meioses
                    const uint64_t up_a = (f >= 0 && j >= 1) ? memo_u[f][j - 1] : 0, up_b = (m >= 0 && j >= 1) ? memo_u[m][j - 1] : 0;
                    v[j] = j == 0 ? 1 : up_a + up_b;
                }
                }
            }
            for (int32_t j : cols_of[x]) {
                if (family == kOcc) v[j] += 1;
                else v[j] = 1;                                                             // rec: the bit; meioses: 0 meioses, stored + 1
            }
            memo_u[x] = v;
        }
        done[x] = 1;
    }
};

int depth_of(const Ped &p, int x, std::vector<int> &memo)
{
    if (memo[x]) return memo[x];
    const int f = p.fa[x] >= 0 ? depth_of(p, p.fa[x], memo) : 0, m = p.mo[x] >= 0 ? depth_of(p, p.mo[x], memo) : 0;
    return memo[x] = 1 + std::max(f, m);
}

// ---- one schedule ------------------------------------------------------------------------------------------------------------------

using ItemKey = std::tuple<int32_t, int32_t, int32_t, int, std::vector<int32_t>>;      // (result row or -1, class A, class B, copy, one-hot columns)

bool check_schedule(const Ped &p, const std::vector<int64_t> &pro_ids, const std::vector<int64_t> &anc_ids_in, const OptSet &os)
{
    const SweepOptions &o = os.o;
    const int n = p.n();
    const std::vector<int64_t> none;
    const std::vector<int64_t> &anc_ids = o.every_member ? none : anc_ids_in;            // completeness has no ancestor list
    ++g.schedules;
    std::vector<int64_t> fa_id(n), mo_id(n);
    for (int i = 0; i < n; ++i) {
        fa_id[i] = p.fa[i] >= 0 ? p.id[p.fa[i]] : 0;
        mo_id[i] = p.mo[i] >= 0 ? p.id[p.mo[i]] : 0;
    }
    SweepSchedule h;
    std::string err;
    const int rc = genphi::plan_sweep(h, n, p.id.data(), fa_id.data(), mo_id.data(), static_cast<int64_t>(pro_ids.size()), pro_ids.data(),
                                      static_cast<int64_t>(anc_ids.size()), anc_ids.data(), o, err);
    // what the call should have made of the lists
    std::map<int64_t, int32_t> rank;
    for (int i = 0; i < n; ++i) rank[p.id[i]] = i;
    std::vector<int32_t> pro, anc_rank;
    bool unknown_pro = false, unknown_anc = false, dropped = false;
    for (int64_t v : pro_ids) {
        auto it = rank.find(v);
        if (it != rank.end()) pro.push_back(it->second);
        else if (o.drop_unknown_pro) dropped = true;
        else unknown_pro = true;
    }
    for (int64_t v : anc_ids) {
        auto it = rank.find(v);
        if (it != rank.end()) anc_rank.push_back(it->second);
        else unknown_anc = true;
    }
    if (unknown_pro || unknown_anc) {
        REQUIRE(rc == GENPHI_ERR_UNKNOWN_ID && !err.empty(), "an unknown ID was not refused with GENPHI_ERR_UNKNOWN_ID", rc);
        if (unknown_pro) ++g.unknown_pro_error; else ++g.unknown_anc_error;
        return true;
    }
    REQUIRE(rc == GENPHI_OK, "plan_sweep failed", rc);
    if (dropped) ++g.unknown_pro_dropped;
    const int n_pro = static_cast<int>(pro.size()), n_anc = static_cast<int>(anc_rank.size());
    const bool emits = o.emit != Emit::None, every = o.every_member;
    REQUIRE(h.n_pro == n_pro && h.n_anc == n_anc, "n_pro / n_anc", h.n_pro, h.n_anc);

    // generations by parent steps from the probands: x is in the cuts at distances tfirst[x] .. tlast[x]
    std::vector<int32_t> distinct, tfirst(n, -1), tlast(n, -1);
    {
        std::vector<char> seen(n, 0);
        for (int32_t x : pro) if (!seen[x]) { seen[x] = 1; distinct.push_back(x); }
    }
    int L = 0;
    {
        std::vector<int32_t> cur = distinct, nxt, stamp(n, -1);
        while (!cur.empty()) {
            nxt.clear();
            for (int32_t x : cur) {
                if (tfirst[x] < 0) tfirst[x] = L;
                tlast[x] = L;
                for (int32_t q : {p.fa[x], p.mo[x]})
                    if (q >= 0 && stamp[q] != L) { stamp[q] = L; nxt.push_back(q); }
            }
            cur.swap(nxt);
            ++L;
        }
    }
    REQUIRE(h.n_steps == std::max(L - 1, 0), "n_steps", h.n_steps, L);
    if (o.emit == Emit::None) {
        REQUIRE(static_cast<int>(h.anc_is_pro.size()) == n_anc, "anc_is_pro size");
        std::vector<char> is_pro(n, 0);
        for (int32_t x : pro) is_pro[x] = 1;
        for (int j = 0; j < n_anc; ++j) REQUIRE((h.anc_is_pro[j] != 0) == (is_pro[anc_rank[j]] != 0), "anc_is_pro", j);
    }
    if (n_pro == 0) ++g.empty_pro;
    if (every && n_pro > 0) ++g.empty_anc_every_member;
    if (n_pro == 0 || (n_anc == 0 && !every)) {
        REQUIRE(h.items.empty() && h.oh_cols.empty() && h.list_begin.empty() && h.list_to_result.empty() && h.pro_slots.empty() &&
                    h.peak_slots == 0 && h.n_generations == 0,
                "an empty request left something in the schedule");
        return true;
    }
    int G = 0;
    if (every) {
        std::vector<int> memo(n, 0);
        for (int32_t x : pro) G = std::max(G, depth_of(p, x, memo));
    }
    REQUIRE(h.n_generations == G, "n_generations", h.n_generations, G);

    // expected one-hot columns and relevance
    std::vector<std::vector<int32_t>> oh_of(n);
    for (int j = 0; j < n_anc; ++j)
        if (!o.first_onehot_only || oh_of[anc_rank[j]].empty()) oh_of[anc_rank[j]].push_back(j);
    std::vector<char> rel(n, 0);
    for (int i = 0; i < n; ++i)
        rel[i] = every || !oh_of[i].empty() || (p.fa[i] >= 0 && rel[p.fa[i]]) || (p.mo[i] >= 0 && rel[p.mo[i]]);
    // result rows of each proband: every listed occurrence, LeafFirst the first one
    std::vector<std::vector<int32_t>> rows_of(n);
    for (int k = 0; k < n_pro; ++k)
        if (o.emit == Emit::EveryProband || rows_of[pro[k]].empty()) rows_of[pro[k]].push_back(k);
    auto emitted = [&](int32_t x) { return rel[x] && (o.emit == Emit::EveryProband || !p.has_child[x]); };

    // the lists as a structure
    const int64_t n_items = static_cast<int64_t>(h.items.size());
    REQUIRE(static_cast<int>(h.list_to_result.size()) == L && static_cast<int>(h.list_begin.size()) == L + 1 &&
                static_cast<int>(h.list_srcs.size()) == L,
            "one list per cut", static_cast<long>(h.list_to_result.size()), L);
    REQUIRE(h.list_begin[0] == 0 && h.list_begin[L] == n_items, "list_begin does not span the items");
    REQUIRE(n_items > 0 && h.items[0].oh == 0, "the first one-hot offset");
    for (int64_t i = 0; i + 1 < n_items; ++i) REQUIRE(h.items[i].oh <= h.items[i + 1].oh, "one-hot offsets decrease", i);
    REQUIRE(h.items[n_items - 1].oh == static_cast<int32_t>(h.oh_cols.size()), "the one-hot offsets do not close at oh_cols.size()");
    const int32_t S = static_cast<int32_t>(h.peak_slots);
    REQUIRE(h.peak_slots >= 0 && h.peak_slots <= n, "peak_slots", h.peak_slots);
    if (every) REQUIRE(h.oh_cols.empty(), "one-hot columns with every_member");

    // classes: members that are new in the same cut with the same relevant parents and the same one-hot columns have equal rows and are
    // interchangeable; everything else must be told apart
    std::map<std::tuple<int, int32_t, int32_t, std::vector<int32_t>>, int32_t> class_of_desc;
    std::vector<int32_t> cls(n, -1);
    std::vector<std::vector<int32_t>> new_in(L);
    for (int i = 0; i < n; ++i)
        if (tlast[i] >= 0) new_in[L - 1 - tlast[i]].push_back(i);
    auto in_cut = [&](int32_t x, int c) { return tlast[x] >= 0 && tfirst[x] <= L - 1 - c && L - 1 - c <= tlast[x]; };
    auto parents_key = [&](int32_t x, int32_t &ca, int32_t &cb) {
        ca = p.fa[x] >= 0 && rel[p.fa[x]] ? cls[p.fa[x]] : -1;
        cb = p.mo[x] >= 0 && rel[p.mo[x]] ? cls[p.mo[x]] : -1;
        if (ca > cb) std::swap(ca, cb);
    };

    const int W = every ? G : n_anc;
    std::vector<Row> slot_u(os.arith == kGC ? 0 : S, Row(W, 0)), res_u;
    std::vector<std::vector<double>> slot_d(os.arith == kGC ? S : 0, std::vector<double>(W, 0.0)), res_d;
    const uint64_t fill = 0;                                 // gc, occ: zeros; meioses: closeness 0 = -1; completeness: every row is written
    if (os.arith == kGC) res_d.assign(n_pro, std::vector<double>(W, 0.0));
    else res_u.assign(n_pro, Row(W, fill));
    std::vector<char> res_written(n_pro, 0);
    std::vector<int32_t> owner(S, -1), written_in(S, -1);
    int64_t expected_peak = 0, live = 0;

    for (int k = 0; k < L; ++k) {
        const bool to_res = emits && k == L - 1;
        REQUIRE((h.list_to_result[k] != 0) == to_res, "list_to_result", k);
        const int64_t b = h.list_begin[k], e = h.list_begin[k + 1] - 1;
        REQUIRE(e >= b, "a list without its sentinel", k);
        const SweepItem &sen = h.items[e];
        REQUIRE(sen.dst == -1 && sen.a == -1 && sen.b == -1, "the sentinel of a list", k);
        ++g.lists;
        // what this list should hold
        std::vector<ItemKey> want, got;
        int64_t new_rows = 0;
        for (int32_t x : new_in[k]) {
            if (!rel[x]) continue;
            int32_t ca, cb;
            parents_key(x, ca, cb);
            auto desc = std::make_tuple(k, ca, cb, oh_of[x]);
            auto it = class_of_desc.find(desc);
            if (it == class_of_desc.end()) it = class_of_desc.emplace(desc, static_cast<int32_t>(class_of_desc.size())).first;
            cls[x] = it->second;
            if (to_res) {
                if (emitted(x))
                    for (int32_t row : rows_of[x]) want.emplace_back(row, ca, cb, 0, oh_of[x]);
            } else {
                want.emplace_back(-1, ca, cb, 0, oh_of[x]);
                ++new_rows;
            }
        }
        if (to_res && o.emit == Emit::EveryProband)
            for (int32_t x : distinct)
                if (rel[x] && tlast[x] > 0)                                  // dragged into the last cut: copied from its slot
                    for (int32_t row : rows_of[x]) want.emplace_back(row, -1, cls[x], o.mark_copies ? 1 : 0, std::vector<int32_t>());
        expected_peak = std::max(expected_peak, live + new_rows);
        // the items: bounds, sources, destinations
        std::vector<char> is_src(S, 0), is_dst(to_res ? n_pro : S, 0);
        double srcs = 0.0;
        for (int64_t i = b; i < e; ++i) {
            const SweepItem &it = h.items[i];
            REQUIRE(it.a >= -1 && it.a < S && it.b >= -2 && it.b < S, "a source slot out of range", it.a, it.b);
            REQUIRE(it.dst >= 0 && it.dst < (to_res ? n_pro : S), "a destination out of range", it.dst, k);
            REQUIRE(it.b != -2 || (to_res && o.mark_copies && it.a >= 0), "a copy mark where no copy item can be", i);
            REQUIRE(!is_dst[it.dst], "two items of one list share a destination", it.dst, k);
            is_dst[it.dst] = 1;
            std::vector<int32_t> cols(h.oh_cols.begin() + it.oh, h.oh_cols.begin() + h.items[i + 1].oh);
            for (size_t q = 0; q < cols.size(); ++q)
                REQUIRE(cols[q] >= 0 && cols[q] < n_anc && (q == 0 || cols[q - 1] < cols[q]), "one-hot columns of an item not ascending inside the list", i);
            int32_t ca = -1, cb = -1;
            for (int32_t s : {it.a, it.b}) {
                if (s < 0) continue;
                REQUIRE(written_in[s] >= 0 && written_in[s] < k, "a source slot that no earlier list wrote", s, k);
                is_src[s] = 1;
                srcs += 1.0;
            }
            if (it.a >= 0) ca = owner[it.a];
            if (it.b >= 0) cb = owner[it.b];
            if (ca > cb) std::swap(ca, cb);
            got.emplace_back(to_res ? it.dst : -1, ca, cb, it.b == -2 ? 1 : 0, cols);
        }
        if (!to_res)
            for (int64_t i = b; i < e; ++i) REQUIRE(!is_src[h.items[i].dst], "a destination slot that an item of the same list reads", h.items[i].dst, k);
        REQUIRE(h.list_srcs[k] == srcs, "list_srcs", k);
        {
            std::vector<ItemKey> w = want, a = got;
            std::sort(w.begin(), w.end());
            std::sort(a.begin(), a.end());
            REQUIRE(w.size() == a.size(), "a list with other rows than the members of its cut need", static_cast<long>(a.size()), static_cast<long>(w.size()));
            for (size_t q = 0; q < w.size(); ++q)
                REQUIRE(w[q] == a[q], "an item that reads other members than its parents (a slot handed out too early?), or lands in another row", k,
                        std::get<0>(a[q]));
        }
        if (to_res && o.emit == Emit::EveryProband)
            for (int32_t x : distinct)
                if (rel[x] && tlast[x] > 0) g.copy_items[os.arith] += static_cast<long>(rows_of[x].size());
        g.items += e - b;
        // the rows, in the caller's arithmetic (no destination is a source of this list: any order)
        for (int64_t i = b; i < e; ++i) {
            const SweepItem &it = h.items[i];
            const bool copy = it.b == -2;
            if (os.arith == kGC) {
                std::vector<double> v(W);
                for (int j = 0; j < W; ++j) v[j] = 0.5 * ((it.a >= 0 ? slot_d[it.a][j] : 0.0) + (it.b >= 0 ? slot_d[it.b][j] : 0.0));
                for (int32_t q = it.oh; q < h.items[i + 1].oh; ++q) v[h.oh_cols[q]] = 1.0;
                (to_res ? res_d[it.dst] : slot_d[it.dst]) = v;
            } else {
                Row v(W);
                for (int j = 0; j < W; ++j) {
                    const uint64_t a = it.a >= 0 ? slot_u[it.a][j] : 0, bb = it.b >= 0 ? slot_u[it.b][j] : 0;
                    switch (os.arith) {
                    case kOcc: v[j] = a + bb; break;
                    case kRec: v[j] = a | bb; break;
                    case kDist: {                                           // closeness K - d in 16 bits, saturating at 0 = none
                        const uint64_t m = std::max(a, bb), step = copy ? 0 : 1;
                        v[j] = m > step ? m - step : 0;
                    } break;
                    default:
                        if (copy) v[j] = a;
                        else v[j] = j == 0 ? 1 : (it.a >= 0 ? slot_u[it.a][j - 1] : 0) + (it.b >= 0 ? slot_u[it.b][j - 1] : 0);
                    }
                }
                for (int32_t q = it.oh; q < h.items[i + 1].oh; ++q) {
                    uint64_t &c = v[h.oh_cols[q]];
                    if (os.arith == kOcc) c += 1;
                    else if (os.arith == kRec) c = 1;
                    else c = 65535;
                }
                (to_res ? res_u[it.dst] : slot_u[it.dst]) = v;
            }
            if (to_res) { res_written[it.dst] = 1; continue; }
            // the slot now belongs to this item's class (it is no source of this list: later items of the list do not see it)
            int32_t ca = it.a >= 0 ? owner[it.a] : -1, cb = it.b >= 0 ? owner[it.b] : -1;
            if (ca > cb) std::swap(ca, cb);
            const std::vector<int32_t> cols(h.oh_cols.begin() + it.oh, h.oh_cols.begin() + h.items[i + 1].oh);
            const auto found = class_of_desc.find(std::make_tuple(k, ca, cb, cols));
            REQUIRE(found != class_of_desc.end(), "an item of no class", i);        // (the match above found one)
            if (written_in[it.dst] >= 0) ++g.reused_slots;
            written_in[it.dst] = k;
            owner[it.dst] = found->second;
        }
        live = 0;
        for (int i = 0; i < n; ++i) live += rel[i] && in_cut(i, k);
    }
    // slots are live while their member is in the cut a list reads or in the one it writes
    REQUIRE(h.peak_slots == expected_peak, "peak_slots is not the largest number of slots live at once", h.peak_slots, expected_peak);
    if (L == 1 && n_pro > 0) ++g.founders_only[os.arith];

    // the results against the top-down recursion
    TopDown td(p, os.arith, W, anc_rank);
    for (int32_t x : distinct) td.need(x);
    if (!emits) {
        std::vector<int32_t> want_pro;
        for (int32_t x : distinct) if (rel[x]) want_pro.push_back(x);
        REQUIRE(h.pro_slots.size() == want_pro.size(), "pro_slots: not one slot per distinct proband with a row", static_cast<long>(h.pro_slots.size()));
        for (size_t q = 0; q < want_pro.size(); ++q) {
            const int32_t s = h.pro_slots[q];
            REQUIRE(s >= 0 && s < S && written_in[s] >= 0 && owner[s] == cls[want_pro[q]], "pro_slots: a slot that is not its proband's", s);
            for (int j = 0; j < W; ++j) REQUIRE(slot_u[s][j] == td.memo_u[want_pro[q]][j], "rec: a proband's row differs from the recursion", s, j);
            g.entries += W;
        }
        return true;
    }
    REQUIRE(h.pro_slots.empty(), "pro_slots on an emitting schedule");
    for (int k = 0; k < n_pro; ++k) {
        const int32_t x = pro[k];
        if (os.arith == kComp) REQUIRE(res_written[k], "completeness: a proband without its result row", k);
        for (int j = 0; j < W; ++j) {
            if (os.arith == kGC) {
                const bool row = !p.has_child[x] && rows_of[x][0] == k;      // the first occurrence of a leaf
                REQUIRE(res_d[k][j] == (row ? td.memo_d[x][j] : 0.0), "gc: a result entry differs from the recursion", k, j);
            } else if (os.arith == kDist) {
                const int got = static_cast<int16_t>(~static_cast<uint16_t>(res_u[k][j]));               // d = K - c = ~c
                REQUIRE(got == static_cast<int>(td.memo_u[x][j]) - 1, "meioses: a result entry differs from the recursion", k, j);
            } else {
                REQUIRE(res_u[k][j] == td.memo_u[x][j], "occ / completeness: a result entry differs from the recursion", k, j);
            }
        }
        g.entries += W;
    }
    return true;
}

// ---- proband and ancestor lists ------------------------------------------------------------------------------------------------------

std::vector<int64_t> ids_of(const Ped &p, const std::vector<int32_t> &ranks)
{
    std::vector<int64_t> v;
    for (int32_t x : ranks) v.push_back(p.id[x]);
    return v;
}

std::vector<int32_t> founders_of(const Ped &p)
{
    std::vector<int32_t> v;
    for (int i = 0; i < p.n(); ++i) if (p.fa[i] < 0 && p.mo[i] < 0) v.push_back(i);
    return v;
}

std::vector<int32_t> draw_probands(const Ped &p, Rng &r, int kind)
{
    const int n = p.n();
    std::vector<int32_t> v;
    if (kind == 0) return v;                                                  // nobody
    if (kind == 1) {                                                          // everybody: probands at every depth, nobody leaves the cuts
        for (int i = 0; i < n; ++i) v.push_back(i);
        if (r.chance(500)) r.shuffle(v);
        return v;
    }
    if (kind == 2) {                                                          // founders only: one cut
        const std::vector<int32_t> f = founders_of(p);
        const int m = 1 + r.below(static_cast<int>(std::min<size_t>(f.size(), 12)));
        for (int q = 0; q < m; ++q) v.push_back(f[r.below(static_cast<int>(f.size()))]);
        return v;
    }
    // mixed: leaves, members of any depth, founders, repeats, shuffled
    const int m = 1 + r.below(std::min(n, 40));
    for (int q = 0; q < m; ++q) {
        int x = r.below(n);
        if (kind == 3 && r.chance(600))                                       // mostly leaves
            for (int tries = 0; tries < 8 && p.has_child[x]; ++tries) x = r.below(n);
        v.push_back(x);
    }
    const int reps = r.below(4);
    for (int q = 0; q < reps; ++q) v.push_back(v[r.below(static_cast<int>(v.size()))]);
    r.shuffle(v);
    return v;
}

std::vector<int32_t> draw_ancestors(const Ped &p, Rng &r, int kind, const std::vector<int32_t> &pro)
{
    const int n = p.n();
    std::vector<int32_t> v;
    if (kind == 0) return v;
    if (kind == 1) {                                                          // everybody: every row has a one-hot of its own
        for (int i = 0; i < n; ++i) v.push_back(i);
        r.shuffle(v);
        return v;
    }
    if (kind == 2) return founders_of(p);
    const int m = 1 + r.below(std::min(n, 70));
    const std::vector<int32_t> f = founders_of(p);
    for (int q = 0; q < m; ++q) v.push_back(r.chance(500) ? f[r.below(static_cast<int>(f.size()))] : r.below(n));      // related or not
    if (!pro.empty()) v.push_back(pro[r.below(static_cast<int>(pro.size()))]);                                        // an ancestor that is a proband
    const int reps = r.below(3);
    for (int q = 0; q < reps; ++q) v.push_back(v[r.below(static_cast<int>(v.size()))]);
    r.shuffle(v);
    return v;
}

bool check_all_callers(const Ped &p, const std::vector<int64_t> &pro, const std::vector<int64_t> &anc, const std::vector<OptSet> &sets,
                       const std::string &where)
{
    bool ok = true;
    for (const OptSet &os : sets) {
        g_where = where + ", " + os.name;
        ok = check_schedule(p, pro, anc, os) && ok;
    }
    return ok;
}

Ped hand_built(const std::vector<std::pair<int, int>> &parents)
{
    Ped p;
    for (const auto &fm : parents) { p.fa.push_back(fm.first); p.mo.push_back(fm.second); }
    finish(p);
    p.id.resize(p.n());
    for (int i = 0; i < p.n(); ++i) p.id[i] = i + 1;
    p.hole = 1000;
    return p;
}

}  // namespace

int main()
{
    const std::vector<OptSet> sets = caller_options();
    // by construction: a chain with a side branch.  ranks: 0, 1 founders; 2 = (0, 1); 3 = (2, -); 4 = (3, 2) two generations back; 5 lone
    const Ped small = hand_built({{-1, -1}, {-1, -1}, {0, 1}, {2, -1}, {3, 2}, {-1, -1}});
    const auto L = [&](std::initializer_list<int32_t> ranks) { return ids_of(small, std::vector<int32_t>(ranks)); };
    check_all_callers(small, L({0, 1, 5, 0}), L({0, 5, 1, 1}), sets, "founders only (one cut)");
    check_all_callers(small, L({4, 3, 2, 3}), L({0, 2, 1, 3}), sets, "probands dragged into the last cut");
    check_all_callers(small, L({4, 0}), L({0, 4, 5}), sets, "a founder dragged through every cut");
    check_all_callers(small, L({}), L({0, 1}), sets, "no probands");
    check_all_callers(small, L({4, 3}), L({}), sets, "no ancestors");
    check_all_callers(small, L({}), L({}), sets, "no probands, no ancestors");
    {
        std::vector<int64_t> pro = L({4, 2}), anc = L({0, 1});
        pro.insert(pro.begin() + 1, small.hole);
        check_all_callers(small, pro, anc, sets, "an unknown proband");
        check_all_callers(small, {small.hole}, anc, sets, "only an unknown proband");
        anc.push_back(small.hole);
        check_all_callers(small, L({4, 2}), anc, sets, "an unknown ancestor");
    }
    const long by_hand = g.schedules;
    for (int f = 0; f < kFamilies; ++f) {
        if (!g.founders_only[f]) { g_where = sets[f].name; fail("the hand-built cases did not reach a schedule of one cut"); }
        if (f != kGC && f != kRec && !g.copy_items[f]) { g_where = sets[f].name; fail("the hand-built cases did not reach a copy item"); }
    }
    if (!g.empty_pro || !g.empty_anc_every_member || !g.unknown_pro_error || !g.unknown_pro_dropped || !g.unknown_anc_error)
        fail("the hand-built cases did not reach every edge");

    const int kPedigrees = 800;
    for (int c = 0; c < kPedigrees; ++c) {
        Rng r(20261017ull * 1000 + static_cast<uint64_t>(c));
        static const int sizes[] = {1, 2, 3, 5, 9, 17, 40, 90, 160, 260};
        const int n = sizes[r.below(10)] + r.below(12);
        const bool layered = r.chance(500);
        const int back_or_width = layered ? 1 + r.below(std::max(n / 3, 1)) : 1 + r.below(n);
        static const int founder_pm[] = {10, 50, 200, 500};
        static const int one_pm[] = {0, 50, 300};
        static const int self_pm[] = {0, 30, 200};
        Ped p = random_ped(r, n, layered, back_or_width, founder_pm[r.below(4)], one_pm[r.below(3)], self_pm[r.below(3)], r.below(500));
        const int ids = r.below(3);
        label(p, ids, r);
        if (ids == kIdsSparse) ++g.hashed_ids; else ++g.direct_ids;
        for (int rep = 0; rep < 2; ++rep) {
            static const int pro_kinds[] = {0, 1, 1, 2, 3, 3, 3, 4, 4, 4, 4, 4};
            static const int anc_kinds[] = {0, 1, 1, 2, 2, 3, 3, 3, 3, 3};
            const int pk = pro_kinds[r.below(12)], ak = anc_kinds[r.below(10)];
            const std::vector<int32_t> pro_r = draw_probands(p, r, pk);
            std::vector<int64_t> pro = ids_of(p, pro_r), anc = ids_of(p, draw_ancestors(p, r, ak, pro_r));
            if (r.chance(60)) pro.insert(pro.begin() + r.below(static_cast<int>(pro.size()) + 1), p.hole);
            if (r.chance(30)) anc.insert(anc.begin() + r.below(static_cast<int>(anc.size()) + 1), p.hole);
            check_all_callers(p, pro, anc, sets,
                              "pedigree " + std::to_string(c) + " (n = " + std::to_string(n) + ", ids " + std::to_string(ids) + "), lists " +
                                  std::to_string(rep) + " (kinds " + std::to_string(pk) + ", " + std::to_string(ak) + ")");
        }
    }
    long copies = 0, one_cut = 0;
    for (int f = 0; f < kFamilies; ++f) { copies += g.copy_items[f]; one_cut += g.founders_only[f]; }
    if (!g.direct_ids || !g.hashed_ids || !g.reused_slots) fail("the random cases did not reach both ID tables and a reused slot");
    std::printf("sweep schedules: %ld checked (%ld by hand), %ld lists, %ld items (%ld copy items), %ld result entries compared; %ld of one cut, "
                "%ld without probands, %ld with an unknown ID refused, %ld with unknown probands dropped, %ld slots handed out again; %ld violations\n",
                g.schedules, by_hand, g.lists, g.items, copies, g.entries, one_cut, g.empty_pro, g.unknown_pro_error + g.unknown_anc_error,
                g.unknown_pro_dropped, g.reused_slots, g.violations);
    return g.violations ? 1 : 0;
}
