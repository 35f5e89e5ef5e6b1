// plan_device.h -- the plan object and its device state, the error plumbing of the sweep's host code, and what the two translation
// units of the sweep share: genphi_hip.hip (upload, the Float32 kernels and their launches, the skeleton of a sweep, the C ABI) and
// sweep_f64.hip (the Float64-storage kernels, their buffers and launches).  Everything else sees a plan through resident.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/genphi.h"
#include "devbuf.h"
#include "device_sizes.h"
#include "error.h"
#include "planner.h"
#include "resident.h"
#include "sparse_levels.h"
#include "tuning.h"

using genphi::DevBuf;
using genphi::LevelStep;
using genphi::Plan;
using genphi::Tuning;          // the hooks of a plan, read once when it is created (tuning.h)
using genphi::PhaseTrace;      // GENPHI_TRACE=1: wall-clock marks of the phases of a call on stderr (planner.h)

inline int fail(int code, const std::string &msg) { return genphi_set_error(code, msg); }

#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(GENPHI_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));  \
    } while (0)

// As HIP_TRY, for an allocation that went through DevBuf::reserve: `what` is the text the message had when the call was spelled out on
// the plan's raw pointer (tests/golden/sweep_host_contract.json pins it) -- frozen message text, not code, as in resident.h.
#define HIP_TRY_AS(what, expr)                                                                  \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(GENPHI_ERR_DEVICE, std::string(what ": ") + hipGetErrorString(e_));     \
    } while (0)

// one entry per level step of levels_small_kernel (genphi_hip.hip)
struct SmallStep {
    const int *srcA, *srcB, *ord;
    int n_prev, n;
};

// Work lists of a SPLIT launch: the hub walk of planner.h (WalkLists) as device arrays.
//   desc : per work row (storage row, output row, B source, rank word)
//   seg  : per segment (first work row, hub row, leading rows without B source, type) + terminators
//   run  : first segment of every run + terminator
// level_split_fast_kernel takes runs as its items, level_split_kernel (grouping-exact: it keeps one 32-bit rank
// mask per child in 4 VGPRs, hence segments of at most 4 children) single segments.
struct DeviceGroups {
    int4 *desc = nullptr, *seg = nullptr;
    int4 *run = nullptr;       // (first segment, hub row | n0 << 16, its rows [z, w)) per run + terminator
    int n_segs = 0, n_runs = 0;
};

struct DeviceStep {
    int *srcA = nullptr, *srcB = nullptr, *ord = nullptr, *work = nullptr;
    unsigned *pk = nullptr;
    DeviceGroups groups;       // SPLIT
    // WIDE: row descriptors of rows_compact_kernel for the cut's own rows (A, B, row, scale exponent)
    // and for the parent rows of Psi_P; the parents' positions; the new rows as a work list
    int4 *rowdesc = nullptr, *pardesc = nullptr;
    int *parents = nullptr, *newrows = nullptr;
    int *pstart = nullptr;     // drag_rows_kernel: first parent of each chunk of 8192 dragged columns
    int *idx = nullptr;        // source column of every dragged member (= srcA; the sources' SLOTS when the source cut is stored by slot:
                               // then rowdesc / pardesc / parents hold slots too, see LevelStep::src_slots)
    int *blk_slot = nullptr;   // (in-place steps) first slot of every granule of 64 new members
    int2 *tiles = nullptr;     // (in-place steps) the kFT-column tiles of the slot ranges that hold dragged members: (first column, end of the range)
    int n_tiles = 0;
    int tile_cols = 256;       // ... their width: 128 for small launches (more, smaller workgroups: cfg3s -2.4 %), 256 otherwise (GENPHI_STAY_TILE forces one)
    int nn = -1;               // index of the new x new sub-step in genphi_plan::nn_steps / nn_dsteps
};

constexpr int kGuardWord = 3;      // d_gcnt[kGuardWord]: the encode guard of a sweep's narrow cuts (group counts use words 0 and 1 of a step's four)

// What exists only while the plan is uploaded.  free_device assigns a default-constructed one: every block goes back to the cache
// (devbuf.h) and every pointer, size, flag and cache key is what it is before the first upload -- a member added here is reset with the rest.
// genphi_plan_device_bytes counts idx_blob, lazy_blobs, d_shard_blob, scratch, buf[], result, final_tmp, psi_p, nn_tmp, d_queues,
// buf64[], result64 and the sparse levels' own figure.  It does NOT count d_glist, d_small, d_cert_p, d_shard_rows / d_shard_out_rows,
// sh_blob and d_perm_rows (small next to the rest; tests/golden/sweep_host_contract.json pins the figure as it is).
struct PlanDevice {
    bool on_device = false;
    int device = -1;
    int n_cus = 256;
    hipStream_t stream = nullptr;
    // The owned blocks, declared in the order in which a release hands them back to the cache (the assignment in free_device goes member
    // by member): the cache evicts its oldest idle blocks first and breaks ties between equal sizes by age, so the order decides which
    // blocks the next plan finds.  Everything else in this struct owns no device memory.
    DevBuf<char> idx_blob;                       // every index array of the upload (BlobPacker); dsteps / nn_dsteps point into it
    std::vector<DevBuf<char>> lazy_blobs;        // walk lists uploaded after the index blob (ensure_groups)
    DevBuf<int> d_shard_rows, d_shard_out_rows;
    DevBuf<char> d_shard_blob;
    DevBuf<int> d_glist;
    DevBuf<int> d_queues;           // 16 work-queue counters per slot (a level step or a new x new sub-step), then d_gcnt and d_cert
    DevBuf<SmallStep> d_small;      // one entry per level step (levels_small_kernel)
    DevBuf<char> sh_blob;
    DevBuf<char> scratch;                        // the queries' staging block (resident_scratch: grown on demand)
    DevBuf<float> buf[2];                        // the two level buffers (sz.buf_of[][c]: which one holds cut c)
    DevBuf<float> result, final_tmp;
    DevBuf<float> psi_p;                         // WIDE: compacted parent matrix Psi[parents][parents]
    DevBuf<int> d_cert_p;                        // certificates of the rows of psi_p ...
    DevBuf<float> nn_tmp;                        // in-place WIDE steps: the new x new block before it is scattered to the new members' slots
    // Float64-storage sweeps (gen.f, pairwise phi): own level matrices and result
    DevBuf<double> buf64[2], result64;
    DevBuf<int> d_perm_rows;                     // storage member of each resident proband row (f64 sweeps)

    std::vector<DeviceStep> dsteps;
    std::vector<const LevelStep *> nn_steps;     // new x new sub-steps of the WIDE steps (owned by the plan's steps)
    std::vector<DeviceStep> nn_dsteps;
    genphi::DeviceSizes sz;                      // buf_of[], cert_cut[], cert_off[] and the buffer sizes of this plan (device_sizes.h)
    int *d_cert_t = nullptr;                     // (inside d_cert_p's block) certificates of the rows of nn_tmp
    size_t cert_p_words = 0;
    int *d_final_perm = nullptr;                 // (inside idx_blob)
    int *d_final_slots = nullptr;                // (the proband cut stayed in place) slot of every proband, result order (inside idx_blob)
    size_t sweep_words = 0;         // ints of d_queues' block (cleared by ONE memset per sweep)
    hipGraphExec_t graph_exec = nullptr;   // captured sweep (see genphi_compute_device)
    // key = (kernel, r0, r1, need_perm, alloc_gen).  A captured graph bakes raw device pointers into
    // its kernel nodes, so every (re)allocation of a buffer the sweep touches bumps alloc_gen:
    // the stale graph can then never be replayed, and a fresh eager run precedes the next capture.
    long long graph_key[5] = {0, 0, 0, 0, 0}, eager_key[5] = {0, 0, 0, 0, 0};
    bool level_bufs_ready = false;         // buf[] / psi_p exist (ensure_level_buffers)
    int level_bufs_from = 0;               // ... buf[] sized for the dense matrices of cuts >= this one (the cuts before it live as row lists)
    bool eager_valid = false;
    DeviceGroups shard_groups;      // SPLIT lists of the last step restricted to the shard (arrays inside d_shard_blob)
    // exactness certificates: one word per row of every level matrix (sz.cert_off[c] = first word of
    // cut c), the per-launch group flags (d_glist) and [certified, other] group counts per step
    int *d_cert = nullptr, *d_gcnt = nullptr;    // (inside d_queues' block)
    // narrow cuts (cut_format.h): the format of every cut in the sweep being enqueued (empty: all Float32), and the host copy of the
    // encode guard -- word kGuardWord of d_gcnt, a spare word of step 0's group counts, cleared with the rest at the start of a sweep
    std::vector<int> cut_fmt;
    unsigned *guard_host = nullptr;              // (pinned; cached_pinned)
    bool guard_pending = false;
    // Row shards: an upper level only needs the rows its shard's last-level rows descend from
    // (~80 % of a cut at 8 shards of cfg4, 55-72 % in the two levels below the last).  Per
    // intermediate step: restricted work list (+ SPLIT descriptors) of the current shard (arrays inside sh_blob).
    struct ShardStep { int *rows = nullptr; DeviceGroups groups; int n_rows = 0; };
    std::vector<ShardStep> sh_steps;
    bool sh_valid = false;
    int64_t shard_r0 = -1, shard_r1 = -1;
    bool stay_active = false;                    // this sweep keeps WIDE levels in place (set per compute call)
    bool res_f64 = false;                        // the resident result is the Float64 one
    int64_t res_ld = 0, res_row_begin = 0, res_n_rows = 0;
    bool res_known = false;                      // a genphi_compute_device call has set the resident row range (it may be empty)
    genphi::OverCache over;                      // genphi_result_over's offsets of the resident result: dropped with it (set_resident_rows)
    // zero-aware leading levels (sparse_levels.h): created and calibrated by the first product sweep of the plan
    genphi::SparseLevels *sparse = nullptr;      // (sparse_levels_destroy; its index arrays live inside idx_blob)
    bool sparse_tried = false;
    std::vector<hipEvent_t> events;
};

// The plan: what the planner made of the pedigree and what survives a release of the device, then the device state (created lazily
// by the first compute)
struct genphi_plan : PlanDevice {
    Plan plan;
    genphi::PlanOptions popt;
    Tuning tun;                                  // environment hooks, read once in genphi_plan_create
    genphi_step_fn step_hook = nullptr;          // genphi_plan_set_step_hook: called before every level step of a Float32 sweep
    void *step_hook_user = nullptr;
    long long alloc_gen = 1;                     // (graph_key; only ever grows: a graph captured before a release is never replayed after it)
    int alloc_count = 0;                         // device allocations of uploads so far (GENPHI_TEST_FAIL_ALLOC)
};

// The constants of one call
struct SweepCall {
    bool f64 = false;                // a Float64-storage sweep (GENPHI_FLAG_STORAGE_F64): sweep_f64.hip
    int kernel = 0;
    int64_t r0 = 0, n_rows = 0;      // the shard: rows [r0, r0 + n_rows) of the proband matrix
    int sparse_k = -1;               // cuts 0..sparse_k are row lists (sparse_levels.h); -1: every level is a dense matrix
    // last step WIDE: the whole level (every row, [dragged, new] storage order) goes to final_tmp, then the shard's rows are delivered in
    // proband order (deliver_proband_order) ...
    bool need_perm = false;
    // ... unless the proband cut STAYED IN PLACE at the end of a run (Plan::final_slots): the last step then writes only the new probands'
    // rows and columns into the run's matrix and the delivery reads from there, by slot -- one pass instead of a compaction + a
    // permutation (genea140 with every individual a proband: the last step 7.7 -> ... ms).  The per-entry sweep (kernel = 1) knows no slots.
    bool last_by_slot = false;
    bool timing = false;
    std::vector<int> ev_after;       // event recorded after step k (timing)
};

// ---- shared by the two units ------------------------------------------------------------------------------
// genphi_hip.hip
hipError_t set_max_lds(const void *fn, size_t bytes);
int ensure_sparse_levels(genphi_plan *p, int kernel, PhaseTrace &trace);
// the events 0 .. n - 1 of a timed sweep exist
int ensure_events(genphi_plan *p, int n);
// Step s <= c.sparse_k of a sweep, whose cuts 0..sparse_k are row lists: a list step, or (s == sparse_k) the step that writes cut s + 1 as
// the dense matrix `dst` and then fetches the lists' error flags.  f64_compact: Float64 entries, rows and columns in the cut's storage
// order over the whole pitch (the Float64 sweep); else Float32 or the narrow format `fmt` with its encode guard (cut_format.h)
int enqueue_list_step(genphi_plan *p, const SweepCall &c, int s, void *dst, bool f64_compact, int fmt, unsigned *guard);
// sweep_f64.hip: the two phases of genphi_compute_device that a Float64-storage sweep does its own way
int prepare_buffers64(genphi_plan *p, SweepCall &c, bool no_sparse, PhaseTrace &trace);
int enqueue_sweep64(genphi_plan *p, const SweepCall &c);
