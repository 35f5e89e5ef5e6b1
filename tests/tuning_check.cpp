// Stand-alone check of csrc/tuning.h, without a GPU (tests/test_tuning_host.py builds and runs it): what tuning_from makes of the text of
// every hook -- defaults, a non-default value each, and the quirks of the parsing -- and what plan_options_from / sparse_tuning_from
// hand on to the planner and the sparse levels.  The expected values are written out here, not derived from the table in tuning.h.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <utility>

#include "../genlib.jl_amd/csrc/tuning.h"

using genphi::Tuning;

static int g_checks = 0, g_violations = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_violations; std::fprintf(stderr, "VIOLATION line %d: %s\n", __LINE__, #cond); } } while (0)

// field by field; `what` names the comparison in a message
static void same(const Tuning &a, const Tuning &b, const char *what)
{
#define F(f) do { ++g_checks; if (!(a.f == b.f)) { ++g_violations; std::fprintf(stderr, "VIOLATION %s: field %s: %lld, expected %lld\n", what, #f, static_cast<long long>(a.f), static_cast<long long>(b.f)); } } while (0)
    F(lds_cap_floats); F(full_max_floats); F(no_stay); F(stay_max_slots); F(stay_headroom); F(stay_mem_pct); F(stay_min_ratio_pct);
    F(stay_slack_pct); F(stay_narrow); F(stay_family); F(colperm_plain); F(stay_last); F(stay_overhead_k); F(stay_narrow_min); F(stay_tile);
    F(stay_scalar_t); F(stay_col_fastest); F(stay_two_pass); F(stay_scatter); F(max_group); F(max_run); F(full_bs); F(no_identity);
    F(cert_min_exp); F(dbg_step); F(no_fast); F(max_cpt); F(fast_nt); F(wide_route); F(tt_noalign); F(no_shard_prune); F(shard_force_step);
    F(shard_force_row); F(shard_prune_min_step); F(no_small); F(no_graph); F(fail_alloc_at); F(sparse_k); F(sparse_permille); F(sparse_min_cut);
    F(sparse_chunk); F(sparse_batch); F(sparse_arena); F(sparse_classes); F(res.d2h_threads); F(res.d2h_pageable); F(res.d2h_sym);
    F(res.d2h_tile_rows); F(res.d2h_tile_cols); F(res.d2h_chunk_mb); F(res.boot_panel); F(res.nearest_buf);
#undef F
}

static Tuning from(std::initializer_list<std::pair<const char *, const char *>> kv)
{
    genphi_tuning tu;
    for (const auto &p : kv) tu.kv[p.first] = p.second;
    return genphi::tuning_from(&tu);
}

// the defaults, written out
static Tuning defaults()
{
    Tuning t;
    t.lds_cap_floats = 0; t.full_max_floats = -1; t.no_stay = false; t.stay_max_slots = 0; t.stay_headroom = -1; t.stay_mem_pct = 0;
    t.stay_min_ratio_pct = -1; t.stay_slack_pct = -1; t.stay_narrow = -1; t.stay_family = -1; t.colperm_plain = false; t.stay_last = -1;
    t.stay_overhead_k = -1; t.stay_narrow_min = -1; t.stay_tile = 0; t.stay_scalar_t = false; t.stay_col_fastest = false; t.stay_two_pass = false;
    t.stay_scatter = false; t.max_group = 8; t.max_run = 1; t.full_bs = 0; t.no_identity = false; t.cert_min_exp = -27; t.dbg_step = -1;
    t.no_fast = false; t.max_cpt = 0; t.fast_nt = 0; t.wide_route = 0; t.tt_noalign = false; t.no_shard_prune = false; t.shard_force_step = -1;
    t.shard_force_row = -1; t.shard_prune_min_step = 0; t.no_small = false; t.no_graph = false; t.fail_alloc_at = 0; t.sparse_k = -2;
    t.sparse_permille = -1; t.sparse_min_cut = -1; t.sparse_chunk = 0; t.sparse_batch = 0; t.sparse_arena = 0; t.sparse_classes = -1;
    t.res.d2h_threads = 0; t.res.d2h_pageable = false; t.res.d2h_sym = -1; t.res.d2h_tile_rows = 0; t.res.d2h_tile_cols = 0; t.res.d2h_chunk_mb = 0;
    t.res.boot_panel = 0; t.res.nearest_buf = 1024;
    return t;
}

static void check_parsing()
{
    same(Tuning(), defaults(), "Tuning()");
    same(from({}), defaults(), "an empty genphi_tuning");

    // every hook at a value that is not its default; presence hooks at "0" and ""
    const Tuning all = from({{"GENPHI_LDS_CAP_FLOATS", "64"}, {"GENPHI_FULL_MAX_FLOATS", "32"}, {"GENPHI_NO_STAY", "1"}, {"GENPHI_STAY_MAX_SLOTS", "5000"},
                             {"GENPHI_STAY_HEADROOM", "2"}, {"GENPHI_STAY_MEM_PCT", "150"}, {"GENPHI_STAY_MIN_RATIO_PCT", "300"}, {"GENPHI_STAY_SLACK_PCT", "10"},
                             {"GENPHI_STAY_NARROW", "2"}, {"GENPHI_STAY_FAMILY", "0"}, {"GENPHI_COLPERM_PLAIN", "0"}, {"GENPHI_STAY_LAST", "0"},
                             {"GENPHI_STAY_OVERHEAD_K", "7"}, {"GENPHI_STAY_NARROW_MIN", "100"}, {"GENPHI_STAY_TILE", "128"}, {"GENPHI_STAY_SCALAR_T", "1"},
                             {"GENPHI_STAY_COL_FASTEST", "2"}, {"GENPHI_STAY_TWO_PASS", "-1"}, {"GENPHI_STAY_SCATTER", "1"}, {"GENPHI_MAX_GROUP", "4"},
                             {"GENPHI_MAX_RUN", "2"}, {"GENPHI_FULL_BS", "128"}, {"GENPHI_NO_IDENTITY", ""}, {"GENPHI_CERT_MIN_EXP", "-5"}, {"GENPHI_DBG_STEP", "3"},
                             {"GENPHI_NO_FAST", "0"}, {"GENPHI_MAX_CPT", "8"}, {"GENPHI_FAST_NT", "512"}, {"GENPHI_WIDE_ROUTE", "b"}, {"GENPHI_TT_NOALIGN", "0"},
                             {"GENPHI_NO_SHARD_PRUNE", "0"}, {"GENPHI_SHARD_FORCE", "3:17"}, {"GENPHI_SHARD_PRUNE_MIN_STEP", "2"}, {"GENPHI_NO_SMALL", "0"},
                             {"GENPHI_NO_GRAPH", "0"}, {"GENPHI_TEST_FAIL_ALLOC", "3"}, {"GENPHI_SPARSE_K", "1"}, {"GENPHI_SPARSE_PERMILLE", "50"},
                             {"GENPHI_SPARSE_MIN_CUT", "10"}, {"GENPHI_SPARSE_CHUNK", "4096"}, {"GENPHI_SPARSE_BATCH", "8"}, {"GENPHI_SPARSE_ARENA", "1000"},
                             {"GENPHI_SPARSE_CLASSES", "1"}, {"GENPHI_D2H_THREADS", "3"}, {"GENPHI_D2H_PAGEABLE", "0"}, {"GENPHI_D2H_SYM", "1"},
                             {"GENPHI_D2H_TILE", "16x64"}, {"GENPHI_D2H_CHUNK_MB", "8"}, {"GENPHI_BOOT_PANEL", "7"}, {"GENPHI_NEAREST_BUF", "100"}});
    Tuning e;
    e.lds_cap_floats = 64; e.full_max_floats = 32; e.no_stay = true; e.stay_max_slots = 5000; e.stay_headroom = 2; e.stay_mem_pct = 150;
    e.stay_min_ratio_pct = 300; e.stay_slack_pct = 10; e.stay_narrow = 2; e.stay_family = 0; e.colperm_plain = true; e.stay_last = 0;
    e.stay_overhead_k = 7; e.stay_narrow_min = 100; e.stay_tile = 128; e.stay_scalar_t = true; e.stay_col_fastest = true; e.stay_two_pass = true;
    e.stay_scatter = true; e.max_group = 4; e.max_run = 2; e.full_bs = 128; e.no_identity = true; e.cert_min_exp = -5; e.dbg_step = 3;
    e.no_fast = true; e.max_cpt = 8; e.fast_nt = 512; e.wide_route = 'B'; e.tt_noalign = true; e.no_shard_prune = true; e.shard_force_step = 3;
    e.shard_force_row = 17; e.shard_prune_min_step = 2; e.no_small = true; e.no_graph = true; e.fail_alloc_at = 3; e.sparse_k = 1;
    e.sparse_permille = 50; e.sparse_min_cut = 10; e.sparse_chunk = 4096; e.sparse_batch = 8; e.sparse_arena = 1000; e.sparse_classes = 1;
    e.res.d2h_threads = 3; e.res.d2h_pageable = true; e.res.d2h_sym = 1; e.res.d2h_tile_rows = 16; e.res.d2h_tile_cols = 64; e.res.d2h_chunk_mb = 8;
    e.res.boot_panel = 7; e.res.nearest_buf = 128;
    same(all, e, "every hook set");

    // the quirks: values that are read as something else, or not at all
    const Tuning q = from({{"GENPHI_NO_STAY", "0"}, {"GENPHI_STAY_SCATTER", "0"}, {"GENPHI_STAY_TWO_PASS", "no"}, {"GENPHI_STAY_COL_FASTEST", "0"},
                           {"GENPHI_STAY_SCALAR_T", ""}, {"GENPHI_STAY_TILE", "200"}, {"GENPHI_MAX_GROUP", "0"}, {"GENPHI_MAX_RUN", "-3"},
                           {"GENPHI_WIDE_ROUTE", "x"}, {"GENPHI_SHARD_FORCE", "3-17"}, {"GENPHI_D2H_TILE", "0x64"}, {"GENPHI_BOOT_PANEL", "-4"},
                           {"GENPHI_NEAREST_BUF", "5000"}, {"GENPHI_LDS_CAP_FLOATS", "abc"}});
    Tuning qe = defaults();
    qe.max_group = 1; qe.max_run = 1; qe.wide_route = 'A'; qe.res.nearest_buf = 4096;
    same(q, qe, "quirks");
    CHECK(from({{"GENPHI_STAY_TILE", "256"}}).stay_tile == 256);
    CHECK(from({{"GENPHI_WIDE_ROUTE", "B"}}).wide_route == 'B' && from({{"GENPHI_WIDE_ROUTE", "a"}}).wide_route == 'A' && from({{"GENPHI_WIDE_ROUTE", ""}}).wide_route == 'A');
    CHECK(from({{"GENPHI_SHARD_FORCE", "5:"}}).shard_force_step == -1 && from({{"GENPHI_SHARD_FORCE", "-2:-9"}}).shard_force_row == -9);
    CHECK(from({{"GENPHI_D2H_TILE", "16"}}).res.d2h_tile_rows == 0 && from({{"GENPHI_D2H_TILE", "8x0"}}).res.d2h_tile_cols == 0 &&
          from({{"GENPHI_D2H_TILE", "1x1"}}).res.d2h_tile_cols == 1);
    CHECK(from({{"GENPHI_NEAREST_BUF", "1000"}}).res.nearest_buf == 512 && from({{"GENPHI_NEAREST_BUF", "0"}}).res.nearest_buf == 1024 &&
          from({{"GENPHI_NEAREST_BUF", "-8"}}).res.nearest_buf == 1024 && from({{"GENPHI_NEAREST_BUF", "4096"}}).res.nearest_buf == 4096);

    // the names: the 50 hooks, each with its prefix; nothing else
    int n = 0;
    for (const char *name : {"GENPHI_LDS_CAP_FLOATS", "GENPHI_FULL_MAX_FLOATS", "GENPHI_NO_STAY", "GENPHI_STAY_MAX_SLOTS", "GENPHI_STAY_HEADROOM", "GENPHI_STAY_MEM_PCT",
                             "GENPHI_STAY_SCATTER", "GENPHI_STAY_TWO_PASS", "GENPHI_STAY_COL_FASTEST", "GENPHI_STAY_SCALAR_T", "GENPHI_STAY_TILE", "GENPHI_STAY_SLACK_PCT",
                             "GENPHI_STAY_MIN_RATIO_PCT", "GENPHI_STAY_NARROW", "GENPHI_STAY_NARROW_MIN", "GENPHI_STAY_OVERHEAD_K", "GENPHI_STAY_LAST", "GENPHI_COLPERM_PLAIN",
                             "GENPHI_STAY_FAMILY", "GENPHI_MAX_GROUP", "GENPHI_MAX_RUN", "GENPHI_FULL_BS", "GENPHI_NO_IDENTITY", "GENPHI_CERT_MIN_EXP", "GENPHI_DBG_STEP",
                             "GENPHI_NO_FAST", "GENPHI_MAX_CPT", "GENPHI_FAST_NT", "GENPHI_WIDE_ROUTE", "GENPHI_TT_NOALIGN", "GENPHI_NO_SHARD_PRUNE", "GENPHI_SHARD_FORCE",
                             "GENPHI_SHARD_PRUNE_MIN_STEP", "GENPHI_NO_SMALL", "GENPHI_NO_GRAPH", "GENPHI_D2H_THREADS", "GENPHI_D2H_PAGEABLE", "GENPHI_D2H_SYM",
                             "GENPHI_D2H_TILE", "GENPHI_D2H_CHUNK_MB", "GENPHI_TEST_FAIL_ALLOC", "GENPHI_SPARSE_K", "GENPHI_SPARSE_PERMILLE", "GENPHI_SPARSE_MIN_CUT",
                             "GENPHI_SPARSE_CHUNK", "GENPHI_SPARSE_CLASSES", "GENPHI_SPARSE_BATCH", "GENPHI_SPARSE_ARENA", "GENPHI_BOOT_PANEL", "GENPHI_NEAREST_BUF"}) {
        CHECK(genphi::tuning_knows(name));
        CHECK(!genphi::tuning_knows(name + 7));
        ++n;
    }
#define COUNT(NAME, SET) +1
    CHECK(n == 50 && (0 GENPHI_TUNING_HOOKS(COUNT)) == 50);
#undef COUNT
    CHECK(!genphi::tuning_knows("GENPHI_NOPE") && !genphi::tuning_knows("GENPHI_ENV_HOOKS") && !genphi::tuning_knows("") && !genphi::tuning_knows("GENPHI_"));
}

static void check_translations()
{
    using genphi::PlanOptions;
    using genphi::SparseTuning;
    {
        // nothing set: the planner's and the sparse levels' own defaults
        const PlanOptions o = genphi::plan_options_from(Tuning(), false), d;
        CHECK(o.full_max_floats == 8192 && o.lds_cap_floats == 36864 && !o.indices_only && !o.no_stay && !o.stay_scatter && o.stay_max_slots == 200000);
        CHECK(o.stay_mem_ratio == 1.2 && o.stay_mem_floor_bytes == 4294967296.0 && o.stay_min_ratio_pct == 200 && o.stay_slack_pct == 6 && o.stay_narrow);
        CHECK(o.stay_step_overhead == 64e6 && o.stay_last && !o.stay_narrow_force && o.stay_narrow_min == 2048 && o.stay_family_order && o.stay_headroom == 0);
        CHECK(o.full_max_floats == d.full_max_floats && o.lds_cap_floats == d.lds_cap_floats && o.stay_max_slots == d.stay_max_slots);
        const SparseTuning s = genphi::sparse_tuning_from(Tuning());
        CHECK(s.max_permille == 200 && s.force_k == -2 && s.min_cut == 1536 && s.chunk_cols == 12288 && s.long_batch == 4 && s.first_entries == (1 << 24) && s.classes == -1);
    }
    {
        Tuning t;
        t.lds_cap_floats = 64; t.full_max_floats = 32; t.no_stay = true; t.stay_scatter = true; t.stay_slack_pct = 10; t.stay_min_ratio_pct = 300;
        t.stay_max_slots = 5000; t.stay_narrow = 2; t.stay_narrow_min = 100; t.stay_overhead_k = 7; t.stay_last = 0; t.stay_family = 0; t.stay_headroom = 2;
        t.stay_mem_pct = 150;
        t.sparse_k = 1; t.sparse_permille = 50; t.sparse_min_cut = 10; t.sparse_chunk = 4096; t.sparse_classes = 1; t.sparse_batch = 8; t.sparse_arena = 1000;
        const PlanOptions o = genphi::plan_options_from(t, true);
        CHECK(o.indices_only && o.lds_cap_floats == 64 && o.full_max_floats == 32 && o.no_stay && o.stay_scatter && o.stay_slack_pct == 10);
        CHECK(o.stay_min_ratio_pct == 300 && o.stay_max_slots == 5000 && o.stay_narrow && o.stay_narrow_force && o.stay_narrow_min == 100);
        CHECK(o.stay_step_overhead == 7000.0 && !o.stay_last && !o.stay_family_order && o.stay_headroom == 2 && o.stay_mem_ratio == 1.5 && o.stay_mem_floor_bytes == 0.0);
        const SparseTuning s = genphi::sparse_tuning_from(t);
        CHECK(s.force_k == 1 && s.max_permille == 50 && s.min_cut == 10 && s.chunk_cols == 4096 && s.classes == 1 && s.long_batch == 8 && s.first_entries == 1000);
    }
    {
        // the thresholds below which a value is not handed on
        Tuning t;
        t.lds_cap_floats = 15; t.full_max_floats = 0; t.stay_slack_pct = 0; t.stay_min_ratio_pct = 0; t.stay_max_slots = 0; t.stay_narrow = 0; t.stay_narrow_min = 0;
        t.stay_overhead_k = 0; t.stay_last = 1; t.stay_family = 1; t.stay_headroom = 0; t.stay_mem_pct = 0;
        t.sparse_k = -1; t.sparse_permille = 0; t.sparse_min_cut = 0; t.sparse_chunk = 0; t.sparse_classes = 0; t.sparse_batch = 5; t.sparse_arena = 0;
        const PlanOptions o = genphi::plan_options_from(t, false);
        CHECK(o.lds_cap_floats == 36864 && o.full_max_floats == 0 && o.stay_slack_pct == 0 && o.stay_min_ratio_pct == 0 && o.stay_max_slots == 200000);
        CHECK(!o.stay_narrow && !o.stay_narrow_force && o.stay_narrow_min == 0 && o.stay_step_overhead == 0.0 && o.stay_last && o.stay_family_order);
        CHECK(o.stay_headroom == 0 && o.stay_mem_ratio == 1.2 && o.stay_mem_floor_bytes == 4294967296.0);
        t.stay_narrow = 1; t.lds_cap_floats = 16;
        const PlanOptions o1 = genphi::plan_options_from(t, false);
        CHECK(o1.stay_narrow && !o1.stay_narrow_force && o1.lds_cap_floats == 16);
        const SparseTuning s = genphi::sparse_tuning_from(t);
        CHECK(s.force_k == -1 && s.max_permille == 200 && s.min_cut == 0 && s.chunk_cols == 12288 && s.classes == 0 && s.long_batch == 4 && s.first_entries == (1 << 24));
        t.sparse_batch = 4;
        CHECK(genphi::sparse_tuning_from(t).long_batch == 4);
    }
    {
        // block_size_for and cert_threshold moved with the type
        Tuning t;
        CHECK(genphi::block_size_for(512, t) == 64 && genphi::block_size_for(513, t) == 256 && genphi::block_size_for(2048, t) == 256 && genphi::block_size_for(2049, t) == 512);
        t.full_bs = 1024;
        CHECK(genphi::block_size_for(10, t) == 1024);
        t.full_bs = 100;
        CHECK(genphi::block_size_for(10, t) == 64);
        Tuning c;
        CHECK(genphi::cert_threshold(c) == 0x31ffffffu);            // bits(2^-27) - 1
        c.cert_min_exp = 0;
        CHECK(genphi::cert_threshold(c) == 0x3f7fffffu);            // bits(1) - 1
        c.cert_min_exp = 5;
        CHECK(genphi::cert_threshold(c) == 0x3f7fffffu);
        c.cert_min_exp = -40;
        CHECK(genphi::cert_threshold(c) == 0x31ffffffu);
    }
}

// without a genphi_tuning the values come from the environment, and only under GENPHI_ENV_HOOKS=1 (which this process sets before the
// first look); a genphi_tuning, even an empty one, shuts the environment out
static void check_environment()
{
    setenv("GENPHI_ENV_HOOKS", "1", 1);
    setenv("GENPHI_MAX_CPT", "8", 1);
    setenv("GENPHI_NO_FAST", "0", 1);
    const Tuning t = genphi::tuning_from(nullptr);
    Tuning e = defaults();
    e.max_cpt = 8; e.no_fast = true;
    same(t, e, "from the environment");
    same(from({}), defaults(), "an empty genphi_tuning under a set environment");
}

int main()
{
    check_parsing();
    check_translations();
    check_environment();
    std::printf("tuning check: %d checks; %d violations\n", g_checks, g_violations);
    return g_violations ? 1 : 0;
}
