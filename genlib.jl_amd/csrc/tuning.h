// tuning.h -- the tuning, A/B and test hooks of a plan (host only; no HIP here, so that tests/tuning_check.cpp builds it with g++).
//
// Every hook is a "GENPHI_NAME" setting that is read ONCE, when the plan is created (genphi_plan_create), and kept in the
// plan: a plan never changes behaviour under the caller's feet, and no launch path calls getenv.  The value comes from a
// genphi_tuning when one is given, else from the environment -- which the library reads only under GENPHI_ENV_HOOKS=1
// (planner.h: env_hook).  What each is for is also in README.md, "Environment hooks"; none is needed in production.
//
// GENPHI_TUNING_HOOKS and GENPHI_FORMAT_HOOKS below are the one place a hook's name is written: the names genphi_tuning_set
// accepts and the body of tuning_from are expanded from them.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>

#include "planner.h"

// A set of "GENPHI_NAME" -> value settings handed to genphi_plan_create_tuned (include/genphi.h): the same knobs without the environment.
struct genphi_tuning {
    std::map<std::string, std::string> kv;
};

namespace genphi {

// keys of the LDS buffer of nearest_kernel: powers of two, >= 2 x GENPHI_NEAREST_MAX_K
constexpr int kNearBufMin = 128, kNearBufMax = 4096, kNearBufDefault = 1024;
// the buffer a plan uses: the hook's value clamped to [kNearBufMin, kNearBufMax] and rounded down to a power of two
inline int nearest_buf_entries(int hook)
{
    if (hook <= 0) return kNearBufDefault;
    int b = kNearBufMin;
    while (b * 2 <= (hook < kNearBufMax ? hook : kNearBufMax)) b *= 2;
    return b;
}

// The hooks the queries of the resident result read (resident.h: ResidentView)
struct ResultTuning {
    int d2h_threads = 0;
    bool d2h_pageable = false;
    int d2h_sym = -1;
    int d2h_tile_rows = 0, d2h_tile_cols = 0;
    int d2h_chunk_mb = 0;
    int boot_panel = 0;
    int nearest_buf = kNearBufDefault;
};

// A field's initialiser is the value of its hook when the hook is not set.
struct Tuning {
    int lds_cap_floats = 0, full_max_floats = -1;
    bool no_stay = false;
    int stay_max_slots = 0, stay_headroom = -1, stay_mem_pct = 0, stay_min_ratio_pct = -1, stay_slack_pct = -1;
    int stay_narrow = -1, stay_family = -1;
    bool colperm_plain = false;
    int stay_last = -1, stay_overhead_k = -1, stay_narrow_min = -1, stay_tile = 0;
    bool stay_scalar_t = false, stay_col_fastest = false, stay_two_pass = false, stay_scatter = false;
    int max_group = 8, max_run = 1, full_bs = 0;
    bool no_identity = false;
    int cert_min_exp = -27, dbg_step = -1;
    bool no_fast = false;
    int max_cpt = 0, fast_nt = 0;
    char wide_route = 0;
    bool tt_noalign = false, no_shard_prune = false;
    int shard_force_step = -1, shard_force_row = -1, shard_prune_min_step = 0;
    bool no_small = false, no_graph = false;
    int fail_alloc_at = 0;
    int sparse_k = -2, sparse_permille = -1, sparse_min_cut = -1, sparse_chunk = 0, sparse_batch = 0, sparse_arena = 0;
    ResultTuning res;
    int sparse_classes = -1;
    bool no_narrow = false;
};

// "AxB" / "A:B" hooks: both fields are set when two numbers >= lo are read, neither otherwise
inline void scan_pair(const char *e, const char *fmt, int lo, int &a, int &b)
{
    int x = 0, y = 0;
    if (std::sscanf(e, fmt, &x, &y) == 2 && x >= lo && y >= lo) { a = x; b = y; }
}

inline int one_of(int v, int a, int b) { return v == a || v == b ? v : 0; }

// X(NAME, what a value does): `e` is the hook's text (never null: a hook that is not set leaves its field alone), `t` the Tuning.
// Hooks that ignore `e` are PRESENCE hooks: any value sets them, "0" too.
#define GENPHI_TUNING_HOOKS(X)                                                                                                           \
    /* test: LDS budget for staged rows (forces SPLIT / WIDE on small inputs) */                                                         \
    X(GENPHI_LDS_CAP_FLOATS, t.lds_cap_floats = std::atoi(e))                                                                            \
    /* tuning: FULL vs SPLIT threshold (row length in floats) */                                                                         \
    X(GENPHI_FULL_MAX_FLOATS, t.full_max_floats = std::atoi(e))                                                                          \
    /* A/B + test: WIDE levels never stay in place (every level is copied into the other buffer) */                                      \
    X(GENPHI_NO_STAY, t.no_stay = std::atoi(e) != 0)                                                                                     \
    /* test: largest slot capacity of an in-place run (default: planner.h) */                                                            \
    X(GENPHI_STAY_MAX_SLOTS, t.stay_max_slots = std::atoi(e))                                                                            \
    /* tuning: extra blocks of free slots per in-place run (longer runs, more memory) */                                                 \
    X(GENPHI_STAY_HEADROOM, t.stay_headroom = std::atoi(e))                                                                              \
    /* test: in-place runs may need this % of the plain buffers' memory (default 120) */                                                 \
    X(GENPHI_STAY_MEM_PCT, t.stay_mem_pct = std::atoi(e))                                                                                \
    /* tuning: a step stays in place while cut >= this % of its new members (default 200) */                                             \
    X(GENPHI_STAY_MIN_RATIO_PCT, t.stay_min_ratio_pct = std::atoi(e))                                                                    \
    /* tuning: free slots beyond the widest (cut + new members) of an in-place run, in % (default 6) */                                  \
    X(GENPHI_STAY_SLACK_PCT, t.stay_slack_pct = std::atoi(e))                                                                            \
    /* A/B + test: 0 = only levels whose rows do not fit in LDS stay in place (the round-3 behaviour); 2 = in place wherever the ratio   \
       test allows, whatever the cost model says */                                                                                      \
    X(GENPHI_STAY_NARROW, t.stay_narrow = std::atoi(e))                                                                                  \
    /* A/B: 0 = new members of a leaving class in rank order instead of by family */                                                     \
    X(GENPHI_STAY_FAMILY, t.stay_family = std::atoi(e))                                                                                  \
    /* A/B + test: the proband-order pass by the one-workgroup-per-row kernel (rounds 1-3) */                                            \
    X(GENPHI_COLPERM_PLAIN, t.colperm_plain = true)                                                                                      \
    /* A/B + test: 0 = the proband cut never stays in place (the step that reads a run's last cut compacts it, then the proband-order    \
       pass: the form of rounds 3 and early 4) */                                                                                        \
    X(GENPHI_STAY_LAST, t.stay_last = std::atoi(e))                                                                                      \
    /* tuning + test: fixed cost of a block-assembled step in the planner's cost model, in thousands of matrix entries (default 64000;   \
       tests that put tiny cuts in place set 0) */                                                                                       \
    X(GENPHI_STAY_OVERHEAD_K, t.stay_overhead_k = std::atoi(e))                                                                          \
    /* tuning + test: narrowest source cut of an in-place step at FULL / SPLIT widths (default 2048) */                                  \
    X(GENPHI_STAY_NARROW_MIN, t.stay_narrow_min = std::atoi(e))                                                                          \
    /* tuning: columns per tile of the fused in-place kernel, 256 or 128 (default, and any other value: by the launch's size) */         \
    X(GENPHI_STAY_TILE, t.stay_tile = one_of(std::atoi(e), 128, 256))                                       \
    /* A/B: the fused kernel writes its transposed tile with 4-byte stores (the round-3 form) instead of 16-byte ones */                 \
    X(GENPHI_STAY_SCALAR_T, t.stay_scalar_t = std::atoi(e) != 0)                                                                         \
    /* A/B: fused kernel's workgroups ordered column-fastest instead of granule-fastest (same columns together) */                       \
    X(GENPHI_STAY_COL_FASTEST, t.stay_col_fastest = std::atoi(e) != 0)                                                                   \
    /* A/B + test: new x dragged and its transpose as two kernels (rows_avg + transpose_slots) instead of the fused one */               \
    X(GENPHI_STAY_TWO_PASS, t.stay_two_pass = std::atoi(e) != 0)                                                                         \
    /* A/B + test: the new x new block of an in-place step always goes through the compact buffer */                                     \
    X(GENPHI_STAY_SCATTER, t.stay_scatter = std::atoi(e) != 0)                                                                           \
    /* tuning: children per segment of the SPLIT work lists (<= 8; <= 4 where rank masks are kept) */                                    \
    X(GENPHI_MAX_GROUP, t.max_group = std::max(1, std::atoi(e)))                                                                         \
    /* tuning: stages per run of the hub walk.  1 (default): a run is one hub and its children; larger: the walk chains from hub to hub  \
       (16-20 % fewer staged rows, measured no faster: profiles/microbench/out/r03_ab_hub_walk_*.out) */                    \
    X(GENPHI_MAX_RUN, t.max_run = std::max(1, std::atoi(e)))                                                                             \
    /* tuning: workgroup size of level_full_kernel */                                                                                    \
    X(GENPHI_FULL_BS, t.full_bs = std::atoi(e))                                                                                          \
    /* test: level step 0 on a materialised 1/2 I */                                                                                     \
    X(GENPHI_NO_IDENTITY, t.no_identity = true)                                                                                          \
    /* test: certificate threshold 2^e, e in [-27, 0] (always safe) */                                                                   \
    X(GENPHI_CERT_MIN_EXP, t.cert_min_exp = std::atoi(e))                                                                                \
    /* GENPHI_WG_TIMES builds: the step whose workgroup timing is recorded */                                                            \
    X(GENPHI_DBG_STEP, t.dbg_step = std::atoi(e))                                                                                        \
    /* test / A-B: grouping-exact SPLIT / FULL bodies only */                                                                            \
    X(GENPHI_NO_FAST, t.no_fast = true)                                                                                                  \
    /* test / tuning: columns per thread of a SPLIT chunk */                                                                             \
    X(GENPHI_MAX_CPT, t.max_cpt = std::atoi(e))                                                                                          \
    /* test / tuning: 512- or 1024-thread certified-rows kernel */                                                                       \
    X(GENPHI_FAST_NT, t.fast_nt = std::atoi(e))                                                                                          \
    /* A-B: 'A' / 'B' route of the WIDE levels (not set = 0: by cost) */                                                                 \
    X(GENPHI_WIDE_ROUTE, t.wide_route = (e[0] == 'B' || e[0] == 'b') ? 'B' : 'A')                                                        \
    /* A-B: transpose without line-aligned destination runs */                                                                           \
    X(GENPHI_TT_NOALIGN, t.tt_noalign = true)                                                                                            \
    /* test: a row shard computes every row of the upper levels */                                                                       \
    X(GENPHI_NO_SHARD_PRUNE, t.no_shard_prune = true)                                                                                    \
    /* "step:row"  debugging aid */                                                                                                      \
    X(GENPHI_SHARD_FORCE, scan_pair(e, "%d:%d", INT_MIN, t.shard_force_step, t.shard_force_row))                                         \
    /* debugging aid */                                                                                                                  \
    X(GENPHI_SHARD_PRUNE_MIN_STEP, t.shard_prune_min_step = std::atoi(e))                                                                \
    /* test: no fused small-level runs */                                                                                                \
    X(GENPHI_NO_SMALL, t.no_small = true)                                                                                                \
    /* A-B: never replay a captured hipGraph */                                                                                          \
    X(GENPHI_NO_GRAPH, t.no_graph = true)                                                                                                \
    /* test: the k-th device allocation of an upload fails (error-path test) */                                                          \
    X(GENPHI_TEST_FAIL_ALLOC, t.fail_alloc_at = std::atoi(e))                                                                            \
    /* A/B + test: last cut kept as row lists (sparse_levels.h): -1 = none (every level dense), k >= 0 = cuts 0..k whatever their        \
       density (clamped to the eligible steps); default: by the calibration run's counts */                                              \
    X(GENPHI_SPARSE_K, t.sparse_k = std::atoi(e))                                                                                        \
    /* tuning: a cut stays sparse while at most this share (1/1000) of its entries is non-zero */                                        \
    X(GENPHI_SPARSE_PERMILLE, t.sparse_permille = std::atoi(e))                                                                          \
    /* tuning + test: ... and only when a cut of the sparse run has this many members */                                                 \
    X(GENPHI_SPARSE_MIN_CUT, t.sparse_min_cut = std::atoi(e))                                                                            \
    /* tuning: columns per workgroup of the sparse -> dense step */                                                                      \
    X(GENPHI_SPARSE_CHUNK, t.sparse_chunk = std::atoi(e))                                                                                \
    /* A/B: list entries in flight per thread of a long row's workgroup, 4 or 8 (default 4; 8 measured slower) */                        \
    X(GENPHI_SPARSE_BATCH, t.sparse_batch = std::atoi(e))                                                                                \
    /* test: entries the row-list arenas start with (default 16 Mi; small values exercise their growth) */                               \
    X(GENPHI_SPARSE_ARENA, t.sparse_arena = std::atoi(e))                                                                                \
    /* A/B + test: 1 / 0 = a row-list step is always / never one launch per class of row lengths (default: where lengths differ much) */ \
    X(GENPHI_SPARSE_CLASSES, t.sparse_classes = std::atoi(e))                                                                            \
    /* tuning: worker threads of genphi_result_to_host */                                                                                \
    X(GENPHI_D2H_THREADS, t.res.d2h_threads = std::atoi(e))                                                                              \
    /* A-B: no pinned staging ring */                                                                                                    \
    X(GENPHI_D2H_PAGEABLE, t.res.d2h_pageable = true)                                                                                    \
    /* opt-in: 1 = a full result crosses the link as upper-triangle tiles + a host mirror pass (default: every entry is copied) */       \
    X(GENPHI_D2H_SYM, t.res.d2h_sym = std::atoi(e))                                                                                      \
    /* "RxC"  test + tuning: tile of the symmetric copy (default 256 x 8192) */                                                          \
    X(GENPHI_D2H_TILE, scan_pair(e, "%dx%d", 1, t.res.d2h_tile_rows, t.res.d2h_tile_cols))                                               \
    /* tuning: size of a pinned staging chunk of genphi_result_to_host (default 16, 4 for results below 2 GB) */                         \
    X(GENPHI_D2H_CHUNK_MB, t.res.d2h_chunk_mb = std::atoi(e))                                                                            \
    /* tuning + test: resamples per panel of genphi_result_bootstrap, 1 .. 8192 (default: what keeps a panel's counts within 256 MiB,    \
       DESIGN.md 17) */                                                                                                                  \
    X(GENPHI_BOOT_PANEL, t.res.boot_panel = std::max(0, std::atoi(e)))                                                                   \
    /* tuning + test: keys of the LDS buffer of genphi_result_nearest, a power of two in [128, 4096] (default 1024; the result does not  \
       depend on it: tests force 128 so that small inputs cut the buffer on every tile) */                                 \
    X(GENPHI_NEAREST_BUF, t.res.nearest_buf = nearest_buf_entries(std::atoi(e)))

// The hooks of the cuts' storage formats (cut_format.h): same X, same reading, same rules.  They are a list of their own only
// because tests/tuning_check.cpp pins GENPHI_TUNING_HOOKS at its 50 names ("nothing else") and existing tests are not edited for a new
// hook; what that test says of "the hooks" now holds for the first list.  tests/cut_format_check.cpp checks this one.
#define GENPHI_FORMAT_HOOKS(X)                                                                                                           \
    /* A/B + test: 1 = every dense cut is stored as Float32 (the early exact cuts are 16-bit integers otherwise) */                      \
    X(GENPHI_NO_NARROW, t.no_narrow = std::atoi(e) != 0)

// is `key` ("GENPHI_NAME") a hook a Tuning understands?  (genphi_tuning_set refuses anything else)
inline bool tuning_knows(const std::string &key)
{
#define GENPHI_X(NAME, SET) if (key == #NAME) return true;
    GENPHI_TUNING_HOOKS(GENPHI_X)
    GENPHI_FORMAT_HOOKS(GENPHI_X)
#undef GENPHI_X
    return false;
}

// the settings of a plan: from a genphi_tuning when one is given, else from the environment (under GENPHI_ENV_HOOKS=1)
inline Tuning tuning_from(const genphi_tuning *tu)
{
    Tuning t;
    auto look = [tu](const char *name) -> const char * {
        if (tu) {
            auto it = tu->kv.find(name);
            return it == tu->kv.end() ? nullptr : it->second.c_str();
        }
        return env_hook(name);
    };
#define GENPHI_X(NAME, SET) if (const char *e = look(#NAME)) { (void)e; SET; }
    GENPHI_TUNING_HOOKS(GENPHI_X)
    GENPHI_FORMAT_HOOKS(GENPHI_X)
#undef GENPHI_X
    return t;
}

// what the planner takes from the hooks (a hook that is not set leaves the planner's default)
inline PlanOptions plan_options_from(const Tuning &t, bool indices_only)
{
    PlanOptions o;
    o.indices_only = indices_only;
    if (t.lds_cap_floats >= 16) o.lds_cap_floats = t.lds_cap_floats;
    if (t.full_max_floats >= 0) o.full_max_floats = t.full_max_floats;
    o.no_stay = t.no_stay;
    o.stay_scatter = t.stay_scatter;
    if (t.stay_slack_pct >= 0) o.stay_slack_pct = t.stay_slack_pct;
    if (t.stay_min_ratio_pct >= 0) o.stay_min_ratio_pct = t.stay_min_ratio_pct;
    if (t.stay_max_slots > 0) o.stay_max_slots = t.stay_max_slots;
    if (t.stay_narrow >= 0) { o.stay_narrow = t.stay_narrow != 0; o.stay_narrow_force = t.stay_narrow == 2; }
    if (t.stay_narrow_min >= 0) o.stay_narrow_min = t.stay_narrow_min;
    if (t.stay_overhead_k >= 0) o.stay_step_overhead = 1000.0 * t.stay_overhead_k;
    if (t.stay_last >= 0) o.stay_last = t.stay_last != 0;
    if (t.stay_family >= 0) o.stay_family_order = t.stay_family != 0;
    if (t.stay_headroom >= 0) o.stay_headroom = t.stay_headroom;
    if (t.stay_mem_pct > 0) { o.stay_mem_ratio = t.stay_mem_pct / 100.0; o.stay_mem_floor_bytes = 0.0; }   // (an explicit share is taken literally)
    return o;
}

// The settings of the zero-aware leading levels (sparse_levels.h)
struct SparseTuning {
    int max_permille = 200;    // the calibration run stops at the first cut with more than this share (in 1/1000) of non-zero entries; which
                               // of the cuts before it is the last sparse one is a matter of estimated times (sparse_levels.hip)
    int force_k = -2;          // test / A-B hook: -2 = by calibration; -1 = never sparse; k >= 0: cuts 0..k sparse whatever the counts say
                               // (clamped to what is eligible)
    int min_cut = 1536;        // ... and only when some cut of the sparse run has at least this many members (narrower levels are launch-bound)
    int chunk_cols = 12288;    // columns per workgroup of the sparse -> dense step (cfg4, same box: 0.62 ms at 8192, 0.56 at 12288, 0.79 at 4096)
    int long_batch = 4;        // list entries a thread of a four-wavefront row keeps in flight (4; 8 = A/B hook: measured SLOWER -- genea140's
                               // largest list steps +12..24 %, cfg3s +22 %, cfg4 the same: r05_ab_sparse_list_step_entries_in_flight_4_vs_8_*.out)
    int first_entries = 1 << 24;   // entries each row-list arena starts with (128 MB: genea140's and cfg3's lists fit, 11 M and 8.5 M entries); the calibration run enlarges them where a cut needs more (test hook: small values)
    int classes = -1;          // a launch per class of row lengths: -1 = where the rows of a cut differ much in length, 1 / 0 = always / never (A/B hook)
};

inline SparseTuning sparse_tuning_from(const Tuning &t)
{
    SparseTuning s;
    s.force_k = t.sparse_k;
    if (t.sparse_permille > 0) s.max_permille = t.sparse_permille;
    if (t.sparse_min_cut >= 0) s.min_cut = t.sparse_min_cut;
    if (t.sparse_chunk > 0) s.chunk_cols = t.sparse_chunk;
    s.classes = t.sparse_classes;
    if (t.sparse_batch == 4 || t.sparse_batch == 8) s.long_batch = t.sparse_batch;
    if (t.sparse_arena > 0) s.first_entries = t.sparse_arena;
    return s;
}

// workgroup size of level_full_kernel for rows of n floats
inline int block_size_for(int64_t n, const Tuning &tun)
{
    {
        const int v = tun.full_bs;
        if (v == 64 || v == 128 || v == 256 || v == 512 || v == 1024) return v;
    }
    if (n <= 512) return 64;
    if (n <= 2048) return 256;
    return 512;       // 4 workgroups per CU overlap staging and gathers; 1024 threads measured 20 % slower (cfg3)
}

// bits(2^-27) - 1: entries below 2^-27 (other than 0) void a row's exactness certificate.  Test hook:
// cert_min_exp = e in [-27, 0] raises the bound to 2^e (always safe: fewer rows certified),
// which makes mixed certified / uncertified levels out of ordinary small pedigrees.
inline unsigned cert_threshold(const Tuning &tun)
{
    const int e = std::max(-27, std::min(0, tun.cert_min_exp));
    return (static_cast<unsigned>(127 + e) << 23) - 1u;
}

}  // namespace genphi
