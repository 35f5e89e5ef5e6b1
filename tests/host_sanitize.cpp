// Host-side sanitizer run ("use -fsanitize=address for the host planner"): the native loader and the planner, the only
// host code on the gen.phi path that indexes by pedigree data, driven over the bundled genealogies and over random pedigrees with
// every planner option, under AddressSanitizer + UndefinedBehaviorSanitizer.  Built and run by tests/test_host_sanitizers.py (CPU
// only; GPU sanitizers are not available on this pool).  Links planner.cpp and loader.cpp directly -- no HIP, no oracle.  Also the host
// tables of genphi_result_group_sums (group_tables.cpp), over label vectors at every edge of theirs, with their invariants checked.
// And the work lists of a row shard (shard_lists.cpp), for five shards of every plan, against a per-row backward closure written here.
//   usage: host_sanitize <genea140.csv> <geneaJi.csv>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../genlib.jl_amd/csrc/device_sizes.h"
#include "../genlib.jl_amd/csrc/group_tables.h"
#include "../genlib.jl_amd/csrc/planner.h"
#include "../genlib.jl_amd/csrc/shard_lists.h"
#include "../include/genphi.h"

static std::string g_err;
int genphi_set_error(int code, const std::string &msg) { g_err = msg; return code; }      // (lives in genphi_hip.hip in the library)

using genphi::Plan;
using genphi::PlanOptions;

static unsigned long long checksum(const Plan &p)
{
    unsigned long long s = static_cast<unsigned long long>(p.n_levels);
    for (int64_t c : p.cut_sizes) s = s * 31u + static_cast<unsigned long long>(c);
    for (const genphi::LevelStep &st : p.steps) {
        s = s * 31u + static_cast<unsigned long long>(st.n + st.n_prev + st.mode);
        for (int32_t v : st.srcA) s += static_cast<unsigned>(v);
        for (int32_t v : st.srcB) s += static_cast<unsigned>(v);
        for (int32_t v : st.work) s += static_cast<unsigned>(v);
    }
    for (int32_t v : p.final_members) s += static_cast<unsigned>(v);
    for (int32_t v : p.final_perm) s += static_cast<unsigned>(v);
    return s;
}

// ---- the work lists of a row shard (shard_lists.h) ------------------------------------------
static int shard_bad(const char *what, const char *why)
{
    std::fprintf(stderr, "shard lists, %s: %s\n", what, why);
    return 1;
}

// What the kernels rely on in a hub walk (planner.h: WalkLists) of `rows` of step s
static int check_walk(const genphi::LevelStep &s, const genphi::WalkLists &w, const std::vector<int> &rows, const int *out_rows, int seg_cap,
                      const char *what)
{
    const int n_rows = static_cast<int>(rows.size()), none = static_cast<int>(s.n_prev);
    if (w.desc4.size() != 4 * rows.size() || w.row_k.size() != rows.size()) return shard_bad(what, "walk: one descriptor per row");
    if (w.seg4.size() < 8 || w.seg4.size() % 4 || w.run.size() < 4 || w.run.size() % 4) return shard_bad(what, "walk: list sizes");
    std::vector<char> seen(rows.size(), 0);
    for (int q = 0; q < n_rows; ++q) {                     // each row exactly once, with its own output row and rank word
        const int k = w.row_k[q];
        if (k < 0 || k >= n_rows || seen[k]) return shard_bad(what, "walk: a row is not listed exactly once");
        seen[k] = 1;
        const int i = rows[k];
        if (w.desc4[4 * q] != i || w.desc4[4 * q + 1] != (out_rows ? out_rows[k] : i) || w.desc4[4 * q + 3] != s.ord[i]) return shard_bad(what, "walk: a descriptor");
    }
    const int n_segs = static_cast<int>(w.seg4.size() / 4) - 2, n_runs = static_cast<int>(w.run.size() / 4) - 1;
    for (int t = n_segs; t < n_segs + 2; ++t)
        if (w.seg4[4 * t] != n_rows || w.seg4[4 * t + 1] || w.seg4[4 * t + 2] || w.seg4[4 * t + 3]) return shard_bad(what, "walk: segment terminators");
    if (w.run[4 * n_runs] != n_segs || w.run[4 * n_runs + 1] || w.run[4 * n_runs + 2] != n_rows || w.run[4 * n_runs + 3] != n_rows) return shard_bad(what, "walk: run terminator");
    if ((n_rows > 0) != (n_segs > 0) || (n_segs > 0) != (n_runs > 0)) return shard_bad(what, "walk: empty lists");
    int next_run = 0;
    for (int g = 0; g < n_segs; ++g) {
        const int b = w.seg4[4 * g], e = w.seg4[4 * g + 4], hub = w.seg4[4 * g + 1], n0 = w.seg4[4 * g + 2], type = w.seg4[4 * g + 3];
        if (b != (g == 0 ? 0 : w.seg4[4 * g - 4 + 4]) || e <= b || e > n_rows) return shard_bad(what, "walk: a segment's rows");
        if (n0 < 0 || n0 > 8 || b + n0 > e || e - b - n0 > seg_cap) return shard_bad(what, "walk: a segment's cap");
        if (hub < 0 || hub > none || type < 0 || type > 2) return shard_bad(what, "walk: a segment's hub or type");
        for (int q = b; q < e; ++q) {
            const int i = w.desc4[4 * q], B = w.desc4[4 * q + 2];
            if (q < b + n0 ? (B != none || s.srcB[i] != none || s.srcA[i] != hub)
                           : (B == none || !((s.srcA[i] == hub && s.srcB[i] == B) || (s.srcB[i] == hub && s.srcA[i] == B)))) return shard_bad(what, "walk: a row's sources");
        }
        if (type == 0) {                                  // a run starts here: its entry repeats the segment
            if (next_run >= n_runs || w.run[4 * next_run] != g || w.run[4 * next_run + 1] != (hub | n0 << 16) || w.run[4 * next_run + 2] != b ||
                w.run[4 * next_run + 3] != e) return shard_bad(what, "walk: a run's entry");
            ++next_run;
        } else {
            if (g == 0) return shard_bad(what, "walk: the first segment continues a run");
            const int prev_hub = w.seg4[4 * g - 3], prev_last_B = w.desc4[4 * (b - 1) + 2];
            if (type == 2 ? hub != prev_hub : hub != prev_last_B) return shard_bad(what, "walk: a continued segment's hub");
        }
    }
    return next_run == n_runs ? 0 : shard_bad(what, "walk: runs without a first segment");
}

// The rows of every cut that rows [r0, r1) of the result descend from: a closure over srcA / srcB from each row on its own (a WIDE
// step reads every row of its source cut, whatever it is asked for); `extra`: one more (cut, member) to start from
static std::vector<std::vector<char>> shard_ancestry(const Plan &pl, int64_t r0, int64_t r1, int extra_cut, int extra_row)
{
    const int n_steps = pl.n_levels - 1;
    std::vector<std::vector<char>> mark(pl.n_levels);
    for (int c = 0; c < pl.n_levels; ++c) mark[c].assign(static_cast<size_t>(pl.cut_sizes[c]), 0);
    std::vector<std::pair<int, int>> stack;
    auto visit = [&](int c, int i) { if (!mark[c][i]) { mark[c][i] = 1; stack.emplace_back(c, i); } };
    auto close = [&] {
        while (!stack.empty()) {
            const std::pair<int, int> t = stack.back();
            stack.pop_back();
            if (t.first == 0) continue;
            const genphi::LevelStep &s = pl.steps[t.first - 1];
            if (s.mode == genphi::kModeWide) continue;     // (its whole source cut is a root below)
            if (s.srcA[t.second] < s.n_prev) visit(t.first - 1, s.srcA[t.second]);
            if (s.srcB[t.second] < s.n_prev) visit(t.first - 1, s.srcB[t.second]);
        }
    };
    for (int st = 0; st < n_steps; ++st)
        if (pl.steps[st].mode == genphi::kModeWide) for (int64_t i = 0; i < pl.steps[st].n_prev; ++i) visit(st, static_cast<int>(i));
    if (extra_cut >= 0) visit(extra_cut, extra_row);
    close();
    for (int64_t r = r0; r < r1; ++r) {
        visit(n_steps, pl.final_perm.empty() ? static_cast<int>(r) : pl.final_perm[r]);
        close();
    }
    return mark;
}

static int check_shard(const Plan &pl, int64_t r0, int64_t r1, const genphi::ShardOptions &opt, const char *what)
{
    genphi::ShardLists sl;
    genphi::build_shard_lists(pl, r0, r1, opt, sl);
    const int n_steps = std::max(pl.n_levels - 1, 0);
    const int64_t n_rows = r1 - r0;
    // the last step: a permutation of the shard, output row = proband - r0
    if (static_cast<int64_t>(sl.rows.size()) != n_rows || sl.out_rows.size() != sl.rows.size()) return shard_bad(what, "last step: list lengths");
    std::vector<char> seen(static_cast<size_t>(n_rows), 0);
    const bool last_wide = n_steps > 0 && pl.steps[n_steps - 1].mode == genphi::kModeWide;
    if (last_wide == pl.final_perm.empty() && n_steps > 0) return shard_bad(what, "final_perm and a WIDE last step go together");
    for (int64_t k = 0; k < n_rows; ++k) {
        const int o = sl.out_rows[k];
        if (o < 0 || o >= n_rows || seen[o]) return shard_bad(what, "last step: output rows are not a permutation");
        seen[o] = 1;
        if (sl.rows[k] != (pl.final_perm.empty() ? static_cast<int>(r0 + o) : pl.final_perm[r0 + o])) return shard_bad(what, "last step: storage row");
        if ((last_wide || n_steps == 0) && o != k) return shard_bad(what, "last step: a WIDE step delivers in proband order");
    }
    const int cap_of[2] = {std::min(opt.max_group, 4), std::min(opt.max_group, 8)};
    if (n_steps > 0 && pl.steps[n_steps - 1].mode == genphi::kModeSplit) {
        const genphi::LevelStep &s = pl.steps[n_steps - 1];
        if (check_walk(s, sl.last_walk, sl.rows, sl.out_rows.data(), cap_of[s.pos_ord], what)) return 1;
    } else if (!sl.last_walk.desc4.empty()) return shard_bad(what, "last step: a walk without a SPLIT step");
    // the upper steps
    const bool pruned = n_rows < pl.n_pro && n_steps >= 2 && !opt.no_prune;
    if (sl.pruned != pruned || sl.upper.size() != (pruned ? static_cast<size_t>(n_steps - 1) : 0)) return shard_bad(what, "pruned or not");
    if (!pruned) return 0;
    const bool forced = opt.force_step >= 0 && opt.force_step < n_steps - 1 && opt.force_row >= 0 && opt.force_row < pl.cut_sizes[opt.force_step + 1] + 1;
    const bool force_none = forced && opt.force_row == pl.cut_sizes[opt.force_step + 1];      // (the "none" row: marked, never in a work list)
    const std::vector<std::vector<char>> mark = shard_ancestry(pl, r0, r1, forced && !force_none ? opt.force_step + 1 : -1, opt.force_row);
    for (int st = n_steps - 2; st >= 0; --st) {
        const genphi::LevelStep &s = pl.steps[st];
        const std::vector<int> &got = sl.upper[st].rows;
        if (s.mode == genphi::kModeWide) {
            if (!got.empty() || !sl.upper[st].walk.desc4.empty()) return shard_bad(what, "a WIDE upper step has a list");
            continue;
        }
        size_t at = 0;                                    // a subsequence of the step's work order that holds exactly the needed rows
        for (int32_t i : s.work) {
            const bool listed = at < got.size() && got[at] == i;
            if (listed != (mark[st + 1][i] != 0)) return shard_bad(what, "an upper step's list is not the needed set, in work order");
            at += listed;
        }
        if (at != got.size()) return shard_bad(what, "an upper step lists rows outside its work order");
        if (pl.steps[st + 1].mode == genphi::kModeWide && (got.size() != s.work.size() || static_cast<int64_t>(got.size()) != s.n))
            return shard_bad(what, "the step above a WIDE step does not hold every row");
        if (s.mode == genphi::kModeSplit) {
            if (check_walk(s, sl.upper[st].walk, got, nullptr, cap_of[s.pos_ord], what)) return 1;
        } else if (!sl.upper[st].walk.desc4.empty()) return shard_bad(what, "an upper walk without a SPLIT step");
    }
    return 0;
}

// five shards of a plan under two sets of walk options, the pruning switched off, and the force hook
static int shards_all_ways(const Plan &pl, const char *what)
{
    const int64_t n = pl.n_pro;
    if (n == 0 || pl.n_levels == 0) return 0;
    const int64_t mid = n / 3 / 4 * 4 + 1;
    const int64_t shards[5][2] = {{0, n}, {0, 1}, {n - 1, n}, {mid, std::max(mid + 1, (n - n / 5) / 4 * 4 + 3)}, {n / 2, n / 2 + 2}};
    int bad = 0;
    for (int v = 0; v < 2 && !bad; ++v) {
        genphi::ShardOptions o;
        if (v == 1) { o.max_group = 3; o.max_run = 4; }
        for (const auto &sh : shards) {
            if (sh[0] < 0 || sh[1] > n || sh[0] >= sh[1]) continue;
            bad |= check_shard(pl, sh[0], sh[1], o, what);
        }
    }
    genphi::ShardOptions off;
    off.no_prune = true;
    bad |= check_shard(pl, 0, 1, off, what);
    // the force hook: one more row of an upper step -- the first one the shard does not need --, the "none" row, a row out of range
    const int n_steps = pl.n_levels - 1;
    if (n > 1 && n_steps >= 2 && !bad) {
        const std::vector<std::vector<char>> mark = shard_ancestry(pl, 0, 1, -1, 0);
        for (int st = n_steps - 2; st >= 0 && st >= n_steps - 4; --st) {
            genphi::ShardOptions f;
            f.force_step = st;
            const std::vector<char> &m = mark[st + 1];
            f.force_row = static_cast<int>(std::find(m.begin(), m.end(), 0) - m.begin());      // (all needed: the "none" row)
            bad |= check_shard(pl, 0, 1, f, what);
            f.force_row = static_cast<int>(m.size()) + 1;
            bad |= check_shard(pl, 0, 1, f, what);
        }
    }
    return bad;
}

// device_sizes.h against what its readers rely on: under both alternations every cut's matrix fits in the buffer it is assigned to (rows + 1,
// or P + 1 when the cut is stored by slot, times the pitch, plus the tail pad) whatever the first dense cut; the certificate offsets increase
// and end at the word total; a cut shares the words of a cut at or before it; the parent matrix and the new x new block hold every sub-step.
static int check_sizes(const Plan &pl, const char *what)
{
    auto bad = [&](const char *why, long long at) { std::fprintf(stderr, "%s: device sizes: %s (at %lld)\n", what, why, at); return 1; };
    const genphi::DeviceSizes z = genphi::device_sizes(pl);
    const int L = pl.n_levels;
    if (static_cast<int>(z.cert_off.size()) != L + 1 || static_cast<int>(z.cert_cut.size()) != L + 1) return bad("table lengths", L);
    if (static_cast<int>(z.buf_of[0].size()) != L || static_cast<int>(z.buf_of[1].size()) != L) return bad("buf_of lengths", L);
    if (L == 0) return (z.cert_off[0] || z.psi_p_floats || z.nn_tmp_floats || z.final_tmp_floats || genphi::result_floats(pl, 0)) ? bad("an empty plan needs memory", 0) : 0;
    size_t words = 0;
    std::vector<size_t> fl(L, 0);
    for (int c = 0; c < L; ++c) {
        const bool by_slot = c + 1 < L && pl.steps[c].src_slots;
        const size_t rows = static_cast<size_t>(by_slot ? pl.steps[c].P : pl.cut_sizes[c]) + 1;
        fl[c] = rows * static_cast<size_t>(pl.ld[c]) + genphi::kTailPadFloats;
        if (z.cert_off[c] != words) return bad("cert_off is not the running row total", c);
        if (z.cert_off[c + 1] <= z.cert_off[c]) return bad("cert_off does not increase", c);
        words += rows;
        if (z.cert_cut[c] < 0 || z.cert_cut[c] > c) return bad("cert_cut[c] > c", c);
        // (what main_ctx reads through cert_cut: the shared words hold every row of the cut)
        if (z.cert_off[z.cert_cut[c] + 1] - z.cert_off[z.cert_cut[c]] < rows && z.cert_cut[c] != c) return bad("a cut has more rows than the certificate words it shares", c);
        for (int v = 0; v < 2; ++v) if (z.buf_of[v][c] != 0 && z.buf_of[v][c] != 1) return bad("buf_of is not 0 / 1", c);
        if (c >= 1 && z.buf_of[1][c] == z.buf_of[1][c - 1]) return bad("the plain alternation does not alternate", c);
        if (c >= 1 && (z.buf_of[0][c] == z.buf_of[0][c - 1]) != pl.steps[c - 1].stay) return bad("a step reads and writes one buffer without staying in place (or the reverse)", c);
    }
    if (z.cert_off[L] != words || z.cert_cut[L] != L) return bad("cert_off does not end at the word total", L);
    for (int first = 0; first < L; ++first) {
        size_t need[2];
        z.level_buffers(first, need);
        for (int c = first; c + 1 < L; ++c)
            for (int v = 0; v < 2; ++v)
                if (need[z.buf_of[v][c]] < fl[c]) return bad("a cut does not fit in its level buffer", c);
        if (first + 1 >= L && (need[0] || need[1])) return bad("level buffers without an intermediate cut", first);
    }
    for (const genphi::LevelStep &st : pl.steps) {
        if (st.mode == genphi::kModeWide && !st.nn.empty()) {
            if (z.psi_p_floats < static_cast<size_t>((st.nn[0].n_prev + 1) * st.nn[0].ld_prev) + genphi::kTailPadFloats) return bad("psi_p too small", st.nn[0].n_prev);
            if (z.psi_p_rows < static_cast<size_t>(st.nn[0].n_prev) + 1) return bad("too few certificate words for psi_p", st.nn[0].n_prev);
        }
        if (st.stay && (z.nn_pad < static_cast<size_t>(st.npad) || z.nn_tmp_floats < static_cast<size_t>(st.npad) * static_cast<size_t>(st.npad) + genphi::kTailPadFloats))
            return bad("nn_tmp too small", st.npad);
    }
    if (z.final_tmp_floats != static_cast<size_t>((pl.n_pro + 1) * pl.ld[L - 1]) + genphi::kTailPadFloats) return bad("final_tmp", L);
    if (genphi::result_floats(pl, pl.n_pro) != static_cast<size_t>(pl.n_pro * pl.ld[L - 1]) || genphi::result_floats(pl, 0) != 0) return bad("result", L);
    return 0;
}

static int plan_all_ways(const std::vector<int64_t> &ind, const std::vector<int64_t> &fa, const std::vector<int64_t> &mo,
                         const std::vector<int64_t> &pro, const char *what)
{
    unsigned long long sum = 0;
    int n_ok = 0;
    for (int variant = 0; variant < 7; ++variant) {
        PlanOptions o;
        if (variant == 1) o.indices_only = true;
        if (variant == 2) o.no_stay = true;
        if (variant == 3) { o.lds_cap_floats = 256; o.full_max_floats = 0; }
        if (variant == 4) { o.stay_scatter = true; o.stay_min_ratio_pct = 110; o.stay_mem_ratio = 1000.0; }
        if (variant == 5) { o.stay_narrow = false; o.full_max_floats = 64; }
        if (variant == 6) { o.lds_cap_floats = 700; o.stay_slack_pct = 0; o.stay_mem_ratio = 1000.0; }
        Plan plan;
        std::string err;
        const int rc = genphi::build_plan(static_cast<int64_t>(ind.size()), ind.data(), fa.data(), mo.data(), static_cast<int64_t>(pro.size()),
                                          pro.data(), o, plan, err);
        if (rc != GENPHI_OK) { std::fprintf(stderr, "%s, variant %d: build_plan failed: %s\n", what, variant, err.c_str()); return 1; }
        sum += checksum(plan);
        if (check_sizes(plan, what)) return 1;
        // the hub walk of every SPLIT step (what the upload builds from the plan)
        for (const genphi::LevelStep &st : plan.steps) {
            if (st.mode != genphi::kModeSplit || st.work.empty()) continue;
            genphi::WalkLists w;
            std::vector<int> rows(st.work.begin(), st.work.end());
            genphi::build_hub_walk(st.srcA.data(), st.srcB.data(), st.ord.data(), static_cast<int32_t>(st.n_prev), rows.data(), nullptr,
                                   static_cast<int>(rows.size()), 4, 1, w);
            for (int32_t v : w.desc4) sum += static_cast<unsigned>(v);
            for (int32_t v : w.run) sum += static_cast<unsigned>(v);
        }
        if (!o.indices_only && shards_all_ways(plan, what)) return 1;      // (an indices-only plan has no work order: no Float32 sweep)
        ++n_ok;
    }
    std::printf("%s: %d plans, checksum %llu\n", what, n_ok, sum);
    return 0;
}

static std::vector<int64_t> probands_of(const std::vector<int64_t> &ind, const std::vector<int64_t> &fa, const std::vector<int64_t> &mo)
{
    std::vector<int64_t> parents(fa);
    parents.insert(parents.end(), mo.begin(), mo.end());
    std::sort(parents.begin(), parents.end());
    std::vector<int64_t> pro;
    for (int64_t x : ind) if (!std::binary_search(parents.begin(), parents.end(), x)) pro.push_back(x);
    return pro;
}

// build_group_tables on one label vector; what the kernels rely on, checked.  Returns 1 on a broken invariant.
static int group_tables_case(const char *what, const std::vector<int32_t> &lab, int G, int64_t r0, int64_t nr, int min_levels = 1)
{
    using namespace genphi;
    const int64_t N = static_cast<int64_t>(lab.size());
    GroupTables t;
    build_group_tables(lab.data(), G, N, r0, nr, 256, t);
    auto bad = [&](const char *why) { std::fprintf(stderr, "group tables, %s: %s\n", what, why); return 1; };
    // counts; the row list holds every labelled resident row once, by group; blocks cut it into <= kGsBlockRows rows of one group
    std::vector<int64_t> n_cols(G, 0), n_rows(G, 0);
    for (int64_t i = 0; i < N; ++i) if (lab[i] >= 0) { ++n_cols[lab[i]]; if (i >= r0 && i < r0 + nr) ++n_rows[lab[i]]; }
    if (t.n_cols != n_cols || t.n_rows != n_rows) return bad("counts");
    std::vector<int> seen_row(static_cast<size_t>(nr), 0);
    size_t at = 0;
    std::vector<int> blocks_of(G, 0);
    for (const GsPair &b : t.blocks) {
        if (b.x != static_cast<int>(at) || b.y < 1 || b.y > kGsBlockRows || at + b.y > t.rowlist.size()) return bad("a block's range");
        const int g = lab[r0 + t.rowlist[at]];
        for (int k = 0; k < b.y; ++k) {
            const int r = t.rowlist[at + k];
            if (r < 0 || r >= nr || lab[r0 + r] != g || (at + k > 0 && lab[r0 + t.rowlist[at + k - 1]] > g)) return bad("a block's rows");
            ++seen_row[r];
        }
        ++blocks_of[g];
        at += b.y;
    }
    if (at != t.rowlist.size()) return bad("the blocks do not cover the row list");
    for (int64_t r = 0; r < nr; ++r) if (seen_row[r] != (lab[r0 + r] >= 0 ? 1 : 0)) return bad("a resident row is not listed exactly once");
    if (t.blocks.empty()) return t.level_rows.empty() && t.list_a.empty() ? 0 : bad("tables without a block");
    // tiles: monotone offsets; every labelled column in exactly one piece of <= kGsPiece columns of its group; every piece in one entry of list B
    if (t.n_tiles != (N + kGsTile - 1) / kGsTile || static_cast<int>(t.tile_lists.size()) != t.n_tiles + 1) return bad("tile count");
    if (t.perm.size() != (t.form ? static_cast<size_t>(t.n_tiles) * kGsTile : 0)) return bad("perm size");
    std::vector<int> seen_col(static_cast<size_t>(N), 0);
    for (int tl = 0; tl < t.n_tiles; ++tl) {
        const GsPair l0 = t.tile_lists[tl], l1 = t.tile_lists[tl + 1];
        if (l1.x < l0.x || l1.y < l0.y || l1.x > static_cast<int>(t.list_a.size()) || l1.y > static_cast<int>(t.list_b.size())) return bad("tile offsets");
        int next_piece = 0;
        std::vector<char> group_in_tile(G, 0);
        for (int i = l0.y; i < l1.y; ++i) {
            const int first = t.list_b[i].x & 0xffff, len = t.list_b[i].x >> 16, g = t.list_b[i].y;
            if (first != next_piece || len < 1 || g < 0 || g >= G || group_in_tile[g]) return bad("list B");
            group_in_tile[g] = 1;
            for (int q = first; q < first + len; ++q) {
                if (l0.x + q >= l1.x) return bad("list B names a piece outside the tile");
                const int w = t.list_a[l0.x + q], c_first = w & 0xffff, c_len = w >> 16;
                if (c_len < 1 || c_len > kGsPiece || c_first + c_len > kGsTile) return bad("a piece's length");
                for (int k = 0; k < c_len; ++k) {
                    const int64_t c = static_cast<int64_t>(tl) * kGsTile + (t.form ? t.perm[static_cast<size_t>(tl) * kGsTile + c_first + k] : c_first + k);
                    if (c >= N || lab[c] != g) return bad("a piece's column");
                    ++seen_col[c];
                }
            }
            next_piece = first + len;
        }
        if (next_piece != l1.x - l0.x) return bad("list B does not cover the tile's pieces");
    }
    if (t.tile_lists[0].x != 0 || t.tile_lists[0].y != 0 || t.tile_lists[t.n_tiles].x != static_cast<int>(t.list_a.size()) ||
        t.tile_lists[t.n_tiles].y != static_cast<int>(t.list_b.size())) return bad("tile offsets' ends");
    for (int64_t c = 0; c < N; ++c) if (seen_col[c] != (lab[c] >= 0 ? 1 : 0)) return bad("a labelled column is not in exactly one piece");
    // slabs and the levels of the reduction: each level's offsets monotone, <= kGsFan rows per output except in the last, which has G rows
    if (t.tiles_per_slab < 1 || t.n_slabs < 1 || static_cast<int64_t>(t.n_slabs) * t.tiles_per_slab < t.n_tiles ||
        static_cast<int64_t>(t.n_slabs - 1) * t.tiles_per_slab >= t.n_tiles || t.n_part != static_cast<int64_t>(t.blocks.size()) * t.n_slabs) return bad("slabs");
    if (t.level_rows.size() != t.level_beg.size() || static_cast<int>(t.level_rows.size()) < min_levels) return bad("levels");
    int64_t in_rows = t.n_part;
    for (size_t l = 0; l < t.level_beg.size(); ++l) {
        const std::vector<int> &beg = t.level_beg[l];
        if (static_cast<int64_t>(beg.size()) != t.level_rows[l] + 1 || beg.front() != 0 || beg.back() != in_rows) return bad("a level's ends");
        for (size_t k = 0; k + 1 < beg.size(); ++k) if (beg[k + 1] < beg[k] || beg[k + 1] - beg[k] > kGsFan) return bad("a level's offsets");
        in_rows = t.level_rows[l];
    }
    if (in_rows != G) return bad("the last level does not have n_groups rows");
    const std::vector<int> &lb = t.level_beg.back();
    if (t.level_beg.size() == 1) for (int g = 0; g < G; ++g) if (lb[g + 1] - lb[g] != blocks_of[g] * t.n_slabs) return bad("a group's rows of part");
    return 0;
}

static int group_tables_all()
{
    int bad = 0;
    auto labels = [](int64_t n, auto f) { std::vector<int32_t> v(static_cast<size_t>(n)); for (int64_t i = 0; i < n; ++i) v[i] = f(i); return v; };
    bad |= group_tables_case("one group, all labelled", labels(100, [](int64_t) { return 0; }), 1, 0, 100);
    bad |= group_tables_case("labels all -1", labels(100, [](int64_t) { return -1; }), 3, 0, 100);
    bad |= group_tables_case("interleaved (form 1)", labels(2500, [](int64_t i) { return i % 7 == 6 ? -1 : static_cast<int>(i % 3); }), 3, 0, 2500);
    bad |= group_tables_case("one run per group (form 0)", labels(2500, [](int64_t i) { return i < 40 ? -1 : static_cast<int>((i - 40) / 500); }), 5, 0, 2500);
    for (int64_t n : {1, 1023, 1024, 1025}) {
        bad |= group_tables_case("N at the tile edge, runs", labels(n, [n](int64_t i) { return static_cast<int>(2 * i / n); }), 2, 0, n);
        bad |= group_tables_case("N at the tile edge, interleaved", labels(n, [](int64_t i) { return static_cast<int>(i % 2); }), 2, 0, n);
    }
    bad |= group_tables_case("a group of 65 rows", labels(200, [](int64_t i) { return i < 65 ? 0 : (i < 129 ? 1 : -1); }), 2, 0, 200);
    bad |= group_tables_case("two levels of the reduction", labels(3000, [](int64_t) { return 0; }), 1, 0, 3000, 2);
    bad |= group_tables_case("two levels, interleaved", labels(5000, [](int64_t i) { return static_cast<int>(i % 2); }), 2, 0, 5000, 2);
    bad |= group_tables_case("a shard that misses a group", labels(900, [](int64_t i) { return static_cast<int>(i / 300); }), 3, 10, 200);
    bad |= group_tables_case("a shard of unlabelled rows", labels(900, [](int64_t i) { return i < 100 ? -1 : 0; }), 1, 0, 100);
    bad |= group_tables_case("an empty shard", labels(900, [](int64_t i) { return static_cast<int>(i % 4); }), 4, 450, 0);
    std::printf("group tables: %s\n", bad ? "FAILED" : "ok");
    return bad;
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: host_sanitize genea140.csv geneaJi.csv\n"); return 2; }
    int bad = group_tables_all();
    for (int f = 1; f <= 2; ++f)
        for (int sort = 0; sort <= 1; ++sort) {
            int64_t n = 0, *ind = nullptr, *fa = nullptr, *mo = nullptr, *sex = nullptr;
            const int rrc = genphi_genealogy_read(argv[f], sort, &n, &ind, &fa, &mo, &sex);
            if (rrc == GENPHI_ERR_ORDER && sort == 0) { std::printf("%s, sort = false: %s (expected: the file lists a child before a parent)\n", argv[f], g_err.c_str()); continue; }
            if (rrc != GENPHI_OK) { std::fprintf(stderr, "read %s: %s\n", argv[f], g_err.c_str()); return 1; }
            std::vector<int64_t> vi(ind, ind + n), vf(fa, fa + n), vm(mo, mo + n), vs(sex, sex + n);
            genphi_free(ind); genphi_free(fa); genphi_free(mo); genphi_free(sex);
            const std::vector<int64_t> pro = probands_of(vi, vf, vm);
            bad |= plan_all_ways(vi, vf, vm, pro, argv[f]);
            // a share of all individuals as probands (ancestors of other probands among them), duplicates, reverse order
            std::vector<int64_t> some;
            for (int64_t k = 0; k < n; k += 7) some.push_back(vi[n - 1 - k]);
            some.push_back(some.front());
            bad |= plan_all_ways(vi, vf, vm, some, "  every seventh individual as a proband");
            // the table again through genphi_genealogy_order, and a branching on the first probands and their founders
            int64_t n2 = 0, *i2 = nullptr, *f2 = nullptr, *m2 = nullptr, *s2 = nullptr;
            if (genphi_genealogy_order(n, vi.data(), vf.data(), vm.data(), vs.data(), 1, &n2, &i2, &f2, &m2, &s2) != GENPHI_OK || n2 != n) { std::fprintf(stderr, "order: %s\n", g_err.c_str()); return 1; }
            genphi_free(i2); genphi_free(f2); genphi_free(m2); genphi_free(s2);
            std::vector<int64_t> few(pro.begin(), pro.begin() + std::min<size_t>(pro.size(), 5));
            if (genphi_branching(n, vi.data(), vf.data(), vm.data(), vs.data(), static_cast<int64_t>(few.size()), few.data(), 0, nullptr, &n2, &i2, &f2, &m2, &s2) != GENPHI_OK) {
                std::fprintf(stderr, "branching: %s\n", g_err.c_str()); return 1;
            }
            std::vector<int64_t> bi(i2, i2 + n2), bf(f2, f2 + n2), bm(m2, m2 + n2);
            genphi_free(i2); genphi_free(f2); genphi_free(m2); genphi_free(s2);
            bad |= plan_all_ways(bi, bf, bm, few, "  branching on five probands");
        }
    // error paths: unknown parent, duplicate ID, unknown proband, a cycle
    {
        const std::vector<int64_t> i{1, 2, 3}, fdup{0, 0, 1}, m0{0, 0, 2};
        int64_t n2 = 0, *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr;
        const std::vector<int64_t> idup{1, 1, 3}, funk{0, 0, 9}, fcyc{3, 0, 1};
        if (genphi_genealogy_order(3, idup.data(), fdup.data(), m0.data(), nullptr, 1, &n2, &a, &b, &c, &d) == GENPHI_OK) { std::fprintf(stderr, "duplicate ID accepted\n"); bad = 1; }
        if (genphi_genealogy_order(3, i.data(), funk.data(), m0.data(), nullptr, 1, &n2, &a, &b, &c, &d) == GENPHI_OK) { std::fprintf(stderr, "unknown father accepted\n"); bad = 1; }
        if (genphi_genealogy_order(3, i.data(), fcyc.data(), m0.data(), nullptr, 1, &n2, &a, &b, &c, &d) == GENPHI_OK) { std::fprintf(stderr, "cycle accepted\n"); bad = 1; }
        Plan plan; std::string err;
        const std::vector<int64_t> pro_unk{7};
        if (genphi::build_plan(3, i.data(), fdup.data(), m0.data(), 1, pro_unk.data(), PlanOptions(), plan, err) == GENPHI_OK) { std::fprintf(stderr, "unknown proband accepted\n"); bad = 1; }
        Plan empty;
        if (genphi::build_plan(3, i.data(), fdup.data(), m0.data(), 0, nullptr, PlanOptions(), empty, err) != GENPHI_OK) { std::fprintf(stderr, "no probands: %s\n", err.c_str()); bad = 1; }
        else bad |= check_sizes(empty, "no probands");
    }
    // random pedigrees: overlapping generations, one-parent individuals, probands at every depth
    std::mt19937_64 rng(20261005);
    for (int rep = 0; rep < 24; ++rep) {
        const int gens = 2 + static_cast<int>(rng() % 14), per = 3 + static_cast<int>(rng() % 400);
        const int skip = static_cast<int>(rng() % 400);
        std::vector<int64_t> ind, fa, mo;
        std::vector<std::vector<int64_t>> g(gens);
        int64_t next = 1;
        for (int k = 0; k < gens; ++k)
            for (int q = 0; q < per; ++q) {
                const int64_t id = next++ * 3 + 1;                       // (IDs that are not positions)
                int64_t f = 0, m = 0;
                if (k > 0) {
                    const int kf = (k >= 2 && static_cast<int>(rng() % 1000) < skip) ? k - 2 : k - 1;
                    const int km = (k >= 2 && static_cast<int>(rng() % 1000) < skip) ? k - 2 : k - 1;
                    f = g[kf][rng() % g[kf].size()]; m = g[km][rng() % g[km].size()];
                    const unsigned u = static_cast<unsigned>(rng() % 100);
                    if (u < 4) f = 0; else if (u < 8) m = 0; else if (u < 10) f = m = 0;
                }
                ind.push_back(id); fa.push_back(f); mo.push_back(m);
                g[k].push_back(id);
            }
        std::vector<int64_t> pro(g[gens - 1]);
        for (int q = 0; q < 6; ++q) pro.push_back(ind[rng() % ind.size()]);
        bad |= plan_all_ways(ind, fa, mo, pro, "random pedigree");
    }
    std::printf(bad ? "FAILED\n" : "host sanitizer run: ok\n");
    return bad;
}
