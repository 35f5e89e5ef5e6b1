/*
 * genphi.h -- C-ABI of the MI355X-native gen.phi hot path (dense kinship matrix).
 *
 * Drop-in boundary.  The reference (GPhMorin/GenLib.jl v0.1.4) has no FFI: its boundary is
 * the Julia method
 *     phi(pedigree::Pedigree, probandIDs::Vector{Int} = pro(pedigree);
 *         verbose::Bool = false, compute::Bool = true)          src/compute.jl:233-304
 * A Julia shim with that exact signature (genlib.jl_amd/julia/GenLibAMD.jl, see
 * INTEGRATION.md) flattens the pedigree the way genout does (src/output.jl:24-29, kept at
 * 64 bit) and `ccall`s the entry points below; tests and bench.py bind the same symbols
 * through ctypes.  Plain pointers and sizes only; nothing throws across this boundary.
 *
 * Each entry point names the reference code it replaces.
 *
 * Conventions
 *   - all arrays are caller-owned; the library copies what it needs and keeps no caller
 *     pointer after a call returns (Julia: GC.@preserve for the duration of the ccall);
 *   - individuals are passed in RANK ORDER (iteration order of the reference's Pedigree,
 *     parents before children, src/create.jl:234-254); parent id 0 = unknown;
 *   - calls on one plan are blocking and must be serialised by the caller; distinct plans
 *     may be used concurrently; HIP streams are private to the plan;
 *   - every function returning int returns GENPHI_OK (0) or an error code; the message is
 *     available from genphi_last_error() (thread-local).
 */
#ifndef GENPHI_H
#define GENPHI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GENPHI_OK               0
#define GENPHI_ERR_UNKNOWN_ID   1   /* reference: KeyError (OrderedDict lookup, src/create.jl:70 via src/compute.jl:196) */
#define GENPHI_ERR_ORDER        2   /* parent listed after its child: KeyError in _finalize_pedigree, src/create.jl:240-241 */
#define GENPHI_ERR_DUPLICATE_ID 3
#define GENPHI_ERR_ALLOC        4
#define GENPHI_ERR_DEVICE       5   /* no usable GPU / HIP failure: the product has NO CPU fallback */
#define GENPHI_ERR_ARG          6

typedef struct genphi_plan genphi_plan;

typedef struct genphi_opts {
    int32_t device;        /* HIP device ordinal; -1 = current device                      */
    int32_t kernel;        /* 0 = default (LDS-staged rows); 1 = naive per-entry gather     */
    int64_t row_begin;     /* final-level row shard [row_begin,row_end) in proband order;   */
    int64_t row_end;       /*   row_end <= 0 means "all rows" (multi-GPU: one shard/rank)   */
    int32_t timing;        /* !=0: record per-level HIP-event timings into genphi_stats     */
    int32_t flags;         /* GENPHI_FLAG_* below, or-ed (0 = defaults)                      */
} genphi_opts;

#define GENPHI_FLAG_NO_GRAPH     1   /* never replay the sweep from a captured hipGraph                         */
#define GENPHI_FLAG_STORAGE_F64  2   /* Float64 level matrices: the values of the reference's Float64 pairwise
                                        recursion (src/compute.jl:66-95) instead of gen.phi's Float32-per-level
                                        matrices; for gen.f / pairwise queries (per-entry kernel, small sets)   */

#define GENPHI_FLAG_NO_SPARSE     4   /* every level as a dense matrix: the leading cuts, whose matrices are almost empty, are
                                        otherwise kept as lists of their non-zero entries (the idea of the reference's second
                                        algorithm, src/compute.jl:391-394; genphi_plan_sparse_levels).  Same values either way. */

#define GENPHI_MAX_STAT_LEVELS 1024
typedef struct genphi_stats {
    int32_t n_steps;                 /* level steps run (L-1)                               */
    int32_t timed;                   /* 1 if the ms fields below were measured              */
    double  total_ms;                /* first level kernel start -> last kernel end (HIP events on the plan's stream) */
    double  final_ms;                /* the last level step (+ proband-order pass) alone    */
    double  perm_ms;                 /* of which: the proband-order column pass (0 if none)  */
    double  algorithmic_bytes;       /* 4 * sum_k (n_k^2 + n_{k+1}^2), SURVEY.md 8(d)       */
    int64_t max_cut;                 /* largest cut size                                    */
    float   level_ms[GENPHI_MAX_STAT_LEVELS]; /* per level step (first n_steps entries)     */
    int64_t level_rows[GENPHI_MAX_STAT_LEVELS]; /* output rows each level step computed (a row shard
                                        computes, above the last level, only the rows it descends from) */
    int32_t nearest_buf;             /* candidate keys a workgroup of genphi_result_nearest holds on this plan (GENPHI_NEAREST_BUF;
                                        the newest field: the struct grows at its end only)  */
} genphi_stats;

/* Replaces the host prologue of phi(): levelisation by parent steps and the cut sets
 * (src/compute.jl:236-251, helper _previous_generation :193-207), plus the index copy
 * (_index_pedigree :165-186, founder_index assignment :287-289) in flat, device-ready form.
 * Pure host work: succeeds without a GPU.
 *   n_ind, ind/father/mother : the pedigree in rank order (0 = unknown parent)
 *   n_pro, pro_ids           : probandIDs (duplicates collapse, as `∩` does at :251)        */
int genphi_plan_create(int64_t n_ind, const int64_t *ind, const int64_t *father,
                       const int64_t *mother, int64_t n_pro, const int64_t *pro_ids,
                       genphi_plan **out);

/* Tuning, A/B and test settings of a plan without the environment.  The library has ~45 knobs (README.md, "Tuning hooks": LDS budget,
 * kernel families, in-place runs, sparse cuts, copy threads ...); none is needed in production.  They can be given as GENPHI_* environment
 * variables -- read ONLY when GENPHI_ENV_HOOKS=1 is set too, so that a library loaded into somebody's process never changes kernels on
 * ambient variables -- or, per plan, through a genphi_tuning: genphi_tuning_set(t, "SPARSE_K", "-1") (the hook's name with or without
 * the GENPHI_ prefix; unknown name -> GENPHI_ERR_ARG).  genphi_plan_create_tuned(..., NULL, ...) = the defaults whatever the
 * environment says.  The plan copies what it needs; the tuning may be destroyed right after.  No reference counterpart.        */
typedef struct genphi_tuning genphi_tuning;
genphi_tuning *genphi_tuning_create(void);
int genphi_tuning_set(genphi_tuning *t, const char *name, const char *value);
void genphi_tuning_destroy(genphi_tuning *t);
int genphi_plan_create_tuned(int64_t n_ind, const int64_t *ind, const int64_t *father,
                             const int64_t *mother, int64_t n_pro, const int64_t *pro_ids,
                             const genphi_tuning *tuning, genphi_plan **out);

/* Level description for the "Step i of n: a founders, b probands, c both." lines
 * (src/compute.jl:253-262 and :280-285).  cut_sizes has *n_levels entries (top founders
 * first, probands last), both_counts has *n_levels-1.  Pointers stay valid until
 * genphi_plan_destroy.                                                                      */
int genphi_plan_levels(const genphi_plan *plan, int32_t *n_levels,
                       const int64_t **cut_sizes, const int64_t **both_counts);

/* Number of distinct probands N (rows/columns of the result, proband first-occurrence order). */
int64_t genphi_plan_n_probands(const genphi_plan *plan);

/* Kernel family the planner chose for level step `step` (0-based, < n_levels-1):
 * 0 = FULL (both source rows of an output row in LDS), 1 = SPLIT (one row at a time),
 * 2 = WIDE (a source row does not fit in LDS: the level is assembled block by block from
 * streaming passes); -1 on a bad argument.  Diagnostic only (tests assert every variant is covered). */
int genphi_plan_step_mode(const genphi_plan *plan, int32_t step);

/* More of the same: info[0] = mode, info[1] = members dragged from the previous cut, info[2] =
 * distinct parents of the new members (WIDE steps, else 0), info[3] = how a WIDE step computes its
 * new x new block: 0 / 1 = a FULL / SPLIT sub-step on the compacted parent matrix, 3 = per-entry
 * kernel (parents too wide as well); -1 for the other modes.                                    */
int genphi_plan_step_info(const genphi_plan *plan, int32_t step, int64_t *info);

/* Diagnostic: how WIDE level step `step` stores its cuts in the Float32 sweep (persistent slots, csrc/planner.h LevelStep::stay).
 * info[0] = 1 when the step writes its cut IN PLACE (members keep their row / column slot in one matrix: only the new rows and
 * columns are written, the dragged x dragged block -- src/compute.jl:108-110 -- is not copied) | 2 when it reads a cut stored by
 * slot | 4 when the new members' slots are one stretch (their new x new block is then written in place instead of scattered);
 * info[1] = slot capacity (row pitch) of that matrix, info[2] / info[3] = first slot / reserved slots of the new members.
 * All zero for every other step.                                                                                               */
int genphi_plan_step_slots(const genphi_plan *plan, int32_t step, int64_t *info);

/* Diagnostic: the work lists of SPLIT level step `step` -- the hub walk over the parent graph of the cut's rows
 * (csrc/planner.h, WalkLists): desc4 = 4 ints per work row (storage row, output row, row to stage or n_prev, rank word),
 * seg4 = 4 ints per segment (first work row, hub row, leading rows without a row to stage, type 0 / 1 / 2) + 2
 * terminators, run4 = 4 ints per run (first segment, hub row | n0 << 16, first and end work row of that segment) + 1
 * terminator.  Call with NULL arrays for the counts.
 * Tests check its invariants (every row once; a type-1 hub is the row staged last; staged rows <= one per child + one per run). */
int genphi_plan_step_walk(const genphi_plan *plan, int32_t step, int64_t *n_rows, int64_t *n_segs, int64_t *n_runs,
                          int32_t *desc4, int32_t *seg4, int32_t *run4);

/* Progress hook for the "Running step k of n (...)" lines the reference prints INSIDE its level loop (src/compute.jl:280-285, verbose):
 * cb(step, n_steps, user) is called on the calling thread right before level step `step` (0-based) is handed to the GPU, in order.
 * While a hook is set the sweep is enqueued launch by launch (never replayed from a captured graph).  cb = NULL removes it.
 * The hook must not call back into the library with the same plan, and must not throw / raise across the C boundary (ctypes swallows
 * a Python exception raised inside it).  A run of tiny steps goes to the GPU as ONE launch: the hooks of all its steps are called, in
 * order, before that launch.                                                                                                     */
typedef void (*genphi_step_fn)(int32_t step, int32_t n_steps, void *user);
int genphi_plan_set_step_hook(genphi_plan *plan, genphi_step_fn cb, void *user);

/* Diagnostic: the zero-aware leading levels of the plan's Float32 sweep.  The level matrices right below the founders are almost
 * empty (Psi = 1/2 I at the top, src/compute.jl:271-274; an entry is non-zero only where two members share an ancestor above), so
 * the sweep keeps cuts 0..k as lists of their non-zero entries -- what the reference's sparse_phi stores, src/compute.jl:391-394 --
 * and step k writes cut k+1 as the first dense matrix.  k is fixed by the first genphi_compute_device of the plan, which counts the
 * non-zero entries of the leading cuts on the GPU.  *k_out = k (-1: every level is dense, or no sweep has run yet); nnz[c] = non-zero
 * entries of cut c for the cuts that were counted (-1 = not counted), entries[c] = the (column, value) pairs cut c is stored as (each
 * non-zero entry once per child of its column: 8 bytes each; what a sparse step reads and writes), at most `cap` of each (either
 * may be NULL); returns how many were filled.                                                                                   */
int genphi_plan_sparse_levels(const genphi_plan *plan, int32_t *k_out, int64_t *nnz, int64_t *entries, int32_t cap);

/* Diagnostic: the storage format of every cut in the plan's last Float32 sweep (0 = Float32, 1 = 16-bit integers in units of
 * 2^-(2c+1), 2 = 24-bit ones): the early dense cuts, whose entries are exactly such integers, are kept narrow between the steps
 * that carry the format (csrc/cut_format.h).  fmt[c] for c < cap; returns how many were filled (0: no sweep has run yet).
 * *guard_out (may be NULL) = the sweep's encode guard: 0 unless an entry of a narrow cut was not such an integer, which is an
 * internal error that genphi_compute_device reports.                                                                          */
int genphi_plan_cut_formats(const genphi_plan *plan, int32_t *fmt, int32_t cap, uint32_t *guard_out);

/* Device memory the plan holds right now, in bytes (level matrices, row lists of the sparse cuts, the resident result, the index
 * arrays): 0 before the first compute and after genphi_plan_release_device.  What a cache of plans budgets with.             */
int64_t genphi_plan_device_bytes(const genphi_plan *plan);

/* Host only: an UPPER BOUND of the device memory a full-result Float32 sweep of this plan allocates (level matrices -- slot matrices of
 * in-place runs included --, the result at ITS pitch, delivery buffers, index arrays, the row-list arenas of the sparse cuts): what a
 * caller compares with the free memory of a GPU before choosing between replicated levels and column panels.  A sweep
 * whose leading cuts run on row lists allocates level matrices only for the cuts that exist as matrices (genea140: 0.35 of 3.2 GB).  */
int64_t genphi_plan_device_bytes_needed(const genphi_plan *plan);

/* 4 * sum_k (n_k^2 + n_{k+1}^2): the algorithmic HBM bytes of one compute. */
double genphi_plan_algorithmic_bytes(const genphi_plan *plan);

/* Replaces src/compute.jl:269-303 (Psi = 1/2 I, the level loop with the per-pair kernel
 * :105-158 under Threads.@threads :291-299, Psi = phi).  Runs on the GPU; the result is
 * left resident in HBM inside the plan (Float32, N x N, proband order, row pitch
 * genphi_result_ld floats).  Float32 storage per level, Float64 accumulation, one RN
 * Float64->Float32 conversion per entry per level: bit-identical to the reference.
 * opts and stats may be NULL.                                                                */
int genphi_compute_device(genphi_plan *plan, const genphi_opts *opts, genphi_stats *stats);

/* Device pointer / row pitch (in floats) / first row and row count of the resident result
 * of the last genphi_compute_device (the rows of the shard it was asked for).  The pitch is a
 * multiple of 64 and at least N, also for an empty shard (n_rows = 0, which is a Float32 result
 * whatever was resident before).                                                             */
int genphi_result_device(const genphi_plan *plan, const float **d_ptr, int64_t *ld,
                         int64_t *row_begin, int64_t *n_rows);

/* Copies the resident rows to host: out is (n_rows x N) dense row-major Float32
 * (== column-major for the symmetric full matrix, so a Julia Matrix{Float32}(undef,N,N)
 * can be passed directly when all rows were computed).                                       */
int genphi_result_to_host(genphi_plan *plan, float *out);

/* Float64 counterpart for results computed with GENPHI_FLAG_STORAGE_F64: out is (n_rows x N) dense
 * row-major Float64.  (genphi_result_to_host on such a result delivers RN32 of these values: one
 * rounding, which is what gen.f returns, src/compute.jl:500-511.)                                  */
int genphi_result_to_host_f64(genphi_plan *plan, double *out);

/* phi(individual_i, individual_j) (src/compute.jl:66-95: the exact Float64 Karigl recursion,
 * un-memoised and exponential on inbred pedigrees) for n_pairs pairs of IDs at once: one Float64
 * level sweep over the individuals named, one lookup per pair.  out[k] = Phi(id_i[k], id_j[k])
 * (id_i[k] == id_j[k] gives the self-kinship 1/2 + Phi(father, mother)/2).  Bit-identical to the
 * recursion while every kinship is exactly representable in Float64 (pedigrees less than ~26
 * generations deep); beyond, within 2 L 2^-53 relative of the exact kinship after L level steps
 * (subnormal results within 4 x 2^-1074, not flushed).  Pedigree arguments as for genphi_plan_create;
 * unknown ID -> GENPHI_ERR_UNKNOWN_ID.                                                              */
int genphi_phi_pairs(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                     int64_t n_pairs, const int64_t *id_i, const int64_t *id_j, double *out, int32_t device);

/* On-device reduction for phiMean(::Matrix{Float32}) (src/compute.jl:454-459) without moving the
 * matrix to the host: Float64 sum of all resident entries and of their diagonal entries.
 * mean off-diagonal kinship = (sum_all - sum_diag) / (N*N - N); with row shards the ranks add
 * their partial sums.  The reference accumulates in Float32 (Julia's pairwise sum), so its
 * value agrees to Float32 rounding, exactly when the sums are exact (geneaJi: 0.171875).      */
int genphi_result_sums(genphi_plan *plan, double *sum_all, double *sum_diag, int64_t *n_rows);

/* The same for sub-populations: the sums of the resident result within and between groups of probands, reduced on the
 * device in one more pass over the matrix.  What phiMean (src/compute.jl:454-459) gives per population when
 * the probands carry a population name, as in the reference's pop140.csv (gen._pop, src/GenLib.jl:76-92).
 *   group[i]          label of proband i (position as in genphi_plan_create, duplicates collapsed): 0 .. n_groups - 1, or
 *                     -1 = in no group; N entries
 *   sums[a][b]        Float64 sum of Phi[i][j] over the RESIDENT rows i of group a and all columns j of group b (n_groups x
 *                     n_groups, row-major; the diagonal entries are included when a == b)
 *   diag[a]           sum of Phi[i][i] over the resident rows of group a
 *   rows_in_group[a]  resident rows of group a; cols_in_group[a]: probands of group a
 *   form              0: every group's probands are one run of the proband order (runs of -1 anywhere); 1: any other labelling.
 *                     Both forms give the same sums up to the order of the additions; form 1 reads a column order from a table.
 * Any output pointer may be NULL.  Mean kinship within group a = (sums[a][a] - diag[a]) / (n_a (n_a - 1)), between a and b =
 * sums[a][b] / (n_a n_b); with row shards the ranks add all four outputs.  The summation order depends on the plan, the
 * resident rows and the labels alone (no floating-point atomics): the same call gives the same bits.  Every term is >= 0, so
 * an entry is within (n - 1) 2^-53 relative of the exact sum of its n Float32 terms, and exact while the terms are dyadic
 * numbers of few bits.  Device memory: tables of a few bytes per proband and partial sums of n_groups + 1 doubles for
 * fewer than 2 (rows / 64 + n_groups) + 24 x compute units row blocks, in the plan's scratch block, kept between calls.
 * An empty shard (no resident row after a genphi_compute_device call) is GENPHI_OK with zero sums, diag and rows_in_group;
 * cols_in_group and form are those of the labels.
 * GENPHI_ERR_ARG: n_groups outside [1, GENPHI_GROUP_SUMS_MAX_GROUPS], a label outside [-1, n_groups), a Float64 result
 * (GENPHI_FLAG_STORAGE_F64); GENPHI_ERR_DEVICE: no resident result.                                                        */
#define GENPHI_GROUP_SUMS_MAX_GROUPS 4096
int genphi_result_group_sums(genphi_plan *plan, int32_t n_groups, const int32_t *group, double *sums, double *diag,
                             int64_t *rows_in_group, int64_t *cols_in_group, int32_t *form);

/* GENLIB's gen.phiOver(phiMatrix, threshold) on the resident result, without moving the matrix: the related pairs, selected on the
 * device in two passes over the upper triangle.  The reference has no phiOver, so this text is the definition.
 *   listed            every pair (i, j) with i in the resident rows [row_begin, row_begin + n_rows), i < j < N and
 *                     (double)Phi[i][j] >= threshold: 0-based positions in proband order (duplicates collapsed as in
 *                     genphi_plan_create), each unordered pair once, never the diagonal, never a padding column of the row pitch
 *   order             by row, then by column; it depends on the result and the threshold alone (no atomics place an entry), so the
 *                     same call returns the same bytes and the lists of consecutive row shards, concatenated, are the full list
 *   threshold         any double but NaN; +infinity lists nothing, -infinity every pair
 *   *n_pairs          always the total count (may be NULL)
 *   rows, cols, values  caller-owned arrays of `cap` entries, each may be NULL.  With cap >= *n_pairs every array given receives
 *                     *n_pairs entries, values[k] being the Float32 entry Phi[rows[k]][cols[k]] bit for bit; with cap < *n_pairs
 *                     nothing is written.  All three NULL is the count-only call: the counting pass alone, one read of the
 *                     upper triangle (2 N^2 bytes); a filling call reads it twice.  The library keeps the per-row counts of the
 *                     last threshold until the result is recomputed or released: a count-only call followed by a filling call
 *                     with the same threshold counts once.
 * An empty result (no resident row, or N < 2) is GENPHI_OK with 0 pairs.  Device memory: 8 bytes per resident row and 12 bytes per
 * listed pair, in the plan's scratch block, kept between calls.
 * GENPHI_ERR_ARG: NULL plan, NaN threshold, cap < 0, a Float64 result (GENPHI_FLAG_STORAGE_F64); GENPHI_ERR_DEVICE: no resident
 * result; GENPHI_ERR_ALLOC: the counts or the list do not fit in device memory (found before the writing pass is launched).  After
 * any error the plan stays usable and the resident result is untouched.                                                          */
int genphi_result_over(genphi_plan *plan, double threshold, int64_t cap, int32_t *rows, int32_t *cols, float *values,
                       int64_t *n_pairs);

/* The k closest relatives of every proband of the resident result, without moving the matrix: an n_rows x k answer that needs no
 * threshold, selected on the device in one pass over the resident rows.  Neither GENLIB nor the reference has such a
 * function, so this text is the definition.  N is the number of probands after duplicates collapse (genphi_plan_create).
 *   candidates        of a resident row i: the columns j in [0, N) with j != i.  Never the diagonal, never a padding column of the
 *                     row pitch.
 *   order             by larger Phi[i][j] first; equal values by smaller j first.  Values are compared as numbers (every entry a
 *                     sweep produces is >= +0), so the order is total and the answer unique.
 *   the k nearest     of row i: the first k candidates in that order, delivered in that order.
 *   k                 1 <= k <= min(N - 1, GENPHI_NEAREST_MAX_K)
 *   cols, values      caller-owned, row-major n_rows x k; either may be NULL, not both.  cols holds 0-based positions in proband
 *                     order, values[r][c] is the Float32 entry Phi[row_begin + r][cols[r][c]] bit for bit.  Row r of the output is
 *                     resident row row_begin + r: the outputs of consecutive row shards, stacked, are the output of the full result.
 * The answer depends on the matrix and k alone (no atomics, nothing depends on the launch geometry or on GENPHI_NEAREST_BUF): the
 * same call returns the same bytes, and the first k' < k columns of a k call are the k' call.
 * An empty shard (no resident row) is GENPHI_OK and writes nothing.  Device memory: 8 n_rows k bytes, in the plan's scratch block,
 * kept between calls.  One read of the resident rows (4 n_rows N bytes).
 * GENPHI_ERR_ARG: NULL plan, both arrays NULL, N < 2, k out of range, a Float64 result (GENPHI_FLAG_STORAGE_F64); GENPHI_ERR_DEVICE:
 * no resident result; GENPHI_ERR_ALLOC: the output does not fit in device memory (found before the launch).  After any error the
 * plan stays usable and the resident result is untouched.                                                                         */
#define GENPHI_NEAREST_MAX_K 64
int genphi_result_nearest(genphi_plan *plan, int32_t k, int32_t *cols, float *values);

/* The product of the resident result with a caller's tall, skinny panel, without moving the matrix: what quadratic
 * forms, projections and iterative solvers over the kinship matrix need.  N is the number of probands after duplicates collapse.
 *   y[r][c]           = sum over j < N of Phi[row_begin + r][j] x[j][c], for the resident rows r and c < k
 *   x                 host, N x k row-major with pitch ldx >= k (in doubles); y: host, n_rows x k with pitch ldy >= k.  The entries of
 *                     y between k and ldy are not written.  1 <= k <= GENPHI_MATMUL_MAX_K.  *n_rows (may be NULL): the resident rows.
 *   arithmetic        Float64 throughout: Phi[i][j] converts exactly, accumulation is by fma, no floating-point atomics.  IEEE
 *                     semantics: 0 x inf is NaN (as in numpy), an entry of Phi that is zero is multiplied like any other.
 *   fixed order       with n4 = N rounded up to a multiple of 4 (the row pitch is a multiple of 64, its padding columns are +0, and
 *                     rows N .. n4 - 1 of the device copy of x are written as +0 on every call): for l = 0 .. 63,
 *                       s_l = the fma chain, from +0, over the columns j < n4 with (j / 4) % 64 == l, in ascending j:
 *                             s <- fma((double)Phi[i][j], x[j][c], s);
 *                     then six rounds t = 32, 16, 8, 4, 2, 1 of s_l <- s_l + s_(l xor t) for all l at once; y = s_0 (every s_l is the
 *                     same by then).  The order depends on N alone: not on k, ldx, ldy or the other columns of the call, not on the
 *                     row's place in a block of rows or on which shard is resident, not on the kernel form that k selects.
 *   consequences      the same call returns the same bits; column c of a k-column call is bit for bit the one-column call on that
 *                     column; the outputs of consecutive row shards, stacked, are the output of the full result bit for bit.
 *                     Any order of N fused terms is within (N + 2) 2^-53 (|Phi| |x|)[r][c] of the exact product, and exact where all
 *                     partial sums are representable (dyadic entries, integer x of moderate size).
 * An empty shard (no resident row after a genphi_compute_device call) is GENPHI_OK, writes nothing to y and sets *n_rows = 0.
 * Device memory: 8 n4 k' bytes for the panel (k' = k rounded up to the column tile: 1, 2, 4, 8 or a multiple of 16) and 8 n_rows k for
 * the product, in the plan's scratch block, kept between calls.  One read of the resident rows for k <= 16, one per 16 columns beyond;
 * 2 n_rows N k Float64 operations.
 * GENPHI_ERR_ARG: NULL plan, NULL x, NULL y while rows are resident, k outside [1, GENPHI_MATMUL_MAX_K], ldx < k, ldy < k, a Float64
 * result (GENPHI_FLAG_STORAGE_F64); GENPHI_ERR_DEVICE: no resident result; GENPHI_ERR_ALLOC: the panel and the product do not fit
 * (found before any launch).  After any error the plan stays usable, the resident result is untouched, and y and *n_rows are not
 * written.                                                                                                                          */
#define GENPHI_MATMUL_MAX_K 64
int genphi_result_matmul(genphi_plan *plan, int32_t k, const double *x, int64_t ldx, double *y, int64_t ldy, int64_t *n_rows);

/* Solves (Phi + ridge I) z = b for k <= GENPHI_MATMUL_MAX_K right-hand sides by conjugate gradients over genphi_result_matmul on the
 * FULL resident result: what the animal model, BLUP and heritability ask of a kinship matrix, (2 Phi s2g + I s2e)^-1 y
 * with ridge = s2e / (2 s2g).  The iteration is a host loop (csrc/result_solve.cpp), one product per iteration for all the columns
 * that still run; every column has its own scalars, and every dot product is a plain ascending Float64 sum on the host, so the same
 * call gives the same bits.
 *   b, z              host, N x k row-major with pitches ldb, ldz >= k; residual (k doubles) and iterations (k) may be NULL
 *   the iteration     per column, with A = Phi + ridge I:  z = 0, r = b, d = b, rho = r.r, nb = sqrt(b.b).  A column with nb == 0 is
 *                     done (z = 0, residual 0, 0 iterations), as is one with nb <= tol nb.  Then, while a column runs and fewer than
 *                     max_iter products were made:  q = Phi d + ridge d;  g = d.q;  if not (g > 0) or g is not finite: the column
 *                     stops with the z it has (breakdown: A is not positive definite along d, or a NaN / inf came in);
 *                     alpha = rho / g;  z += alpha d;  r -= alpha q;  rho' = r.r;  if sqrt(rho') <= tol nb: the column stops
 *                     (converged by the recurrence residual);  d = r + (rho' / rho) d;  rho = rho'.
 *   iterations[c]     the products of the iteration that column c took part in (the breakdown step included)
 *   residual[c]       after the iteration one more product, over the columns that are not zero, gives the TRUE relative residual
 *                     || b - (Phi z + ridge z) ||_2 / || b ||_2; the return value is GENPHI_OK whether or not every column converged:
 *                     residual says (a column converged when residual[c] <= tol, up to the rounding of the products).
 * GENPHI_ERR_ARG: NULL plan, NULL b, NULL z, k outside [1, GENPHI_MATMUL_MAX_K], ldb < k, ldz < k, ridge negative or not finite, tol
 * negative or NaN, max_iter < 1, a Float64 result, fewer than N rows resident (a shard cannot solve; an empty shard too);
 * GENPHI_ERR_DEVICE: no resident result; GENPHI_ERR_ALLOC as for genphi_result_matmul.  After any error the plan stays usable, the
 * resident result is untouched, and z, residual and iterations are not written.                                                    */
int genphi_result_solve(genphi_plan *plan, int32_t k, const double *b, int64_t ldb, double ridge, double tol, int32_t max_iter,
                        double *z, int64_t ldz, double *residual, int32_t *iterations);

/* The k algebraically largest eigenpairs of the FULL resident result, or of its Gower-centred form J Phi J, J = I - 1 1^T / N, by
 * Lanczos with full reorthogonalisation: the principal components / principal coordinates of population structure.
 * Neither GENLIB nor the reference has such a function, so this text is the definition.  The Krylov basis, the working vector and
 * the Ritz vectors live on the device from the first step to the last (the plan's scratch block); per step only the projection
 * coefficients cross the link.  N is the number of probands after duplicates collapse.
 *   Op                x -> Phi x (genphi_result_matmul's one-column product, its bits), or with center != 0 x -> c(Phi c(x)), c the
 *                     subtraction of the mean over the N rows
 *   start vector      a splitmix64 stream on seed (state += 0x9E3779B97F4A7C15; z = state; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *                     z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31):  u = (z >> 11) 2^-53,  x_e = 2 u - 1, e ascending;
 *                     centred when center is set, then normalised (plain ascending Float64 sums on the host)
 *   step m = 1, 2 ..  w = Op v_m;  h = V_m^T w;  w -= V_m h;  h' = V_m^T w;  w -= V_m h'  (classical Gram-Schmidt, twice, against
 *                     all m basis vectors);  alpha_m = h_m + h'_m;  beta_m = ||w||;  v_(m+1) = w (1 / beta_m).  T_m is the
 *                     tridiagonal matrix of the alpha (diagonal) and beta (beside it).
 *   convergence       after every step m >= k: with theta_1 >= theta_2 >= .. the eigenvalues of T_m and s_(m,i) the last components
 *                     of its unit eigenvectors, pair i has converged when beta_m |s_(m,i)| <= tol theta_1.  (The scale is the
 *                     largest Ritz value: the zero eigenvalue of a centred matrix needs no special case.)  The iteration stops when
 *                     the k largest have converged, or after min(max_iter, N) steps.  tol = 0 is allowed.
 *   breakdown         beta_m <= 2^-40 max over i <= m of (|alpha_i| + beta_i): the Krylov space is invariant.  With m >= k the
 *                     iteration stops and every pair counts as converged.  With m < k it goes on with the next N draws of the
 *                     stream as a fresh vector (centred when center is set, normalised), orthogonalised twice against the basis and
 *                     normalised again, and T holds a 0 at that place; if no more than 2^-40 of the fresh vector is left, it stops.
 *   non-finite        an alpha or beta that is not finite (it cannot occur on a kinship matrix) stops the iteration: values, vectors
 *                     and residual are NaN, no flag is set, the return value is GENPHI_OK.  (So does N = 1 with center set: the
 *                     centred start vector is zero and cannot be normalised.)
 *   the pairs         the k largest eigenvalues theta_i of the last T_m, descending, and u_i = V_m s_i (centred once more when center
 *                     is set); the sign of u_i makes its component of largest magnitude, the one of smallest index among equals,
 *                     positive
 *   values            k doubles, descending
 *   vectors           N x k row-major with pitch ldv >= k (in doubles): column i is the unit vector u_i.  Entries between k and ldv
 *                     are not written.
 *   residual          k doubles, may be NULL: the TRUE || Op u_i - theta_i u_i ||_2, from one more k-column product on the device
 *   converged         k flags, may be NULL: the Lanczos estimate above at the last step (all 1 after a breakdown with m >= k)
 *   products          may be NULL: the Lanczos steps taken (one-column products; the residual's k-column product is not counted)
 * REPEATED EIGENVALUES: one Krylov sequence finds ONE vector per distinct eigenvalue.  An eigenvalue that is repeated among the top k
 * is reported once, and the list goes on with the next distinct ones; further copies appear only after a breakdown (Phi = I / 2
 * returns k copies of 1/2 that way) -- or, in floating point, when the iteration runs on long after that eigenvalue has converged:
 * every step leaves rounding noise of the order 2^-53 along the other directions of its eigenspace, the iteration amplifies it as
 * it amplifies any component there, and a copy emerges once the amplification reaches 2^53 (not before the later pairs of the list
 * have converged to about the square root of that, so not at the default tol on a spectrum as crowded as a kinship matrix's).  A
 * block method is not provided.
 * The return value is GENPHI_OK whether or not every pair converged: converged and residual say.
 * Sums on the device have one order, fixed by n4 = N rounded up to 4 alone: thread t of 256 adds the entry pairs (2p, 2p + 1),
 * p = t, t + 256, .., by fma in ascending p; six rounds s_l += s_(l xor t), t = 32 .. 1, inside each of the four waves; then
 * ((s_0 + s_1) + s_2) + s_3.  A combination sum_i c_i v_i is an fma chain in ascending i.  No floating-point atomics: the same call
 * gives the same bytes, whatever an earlier call left in the scratch block.
 * Device memory, in the plan's scratch block (one request, before the first launch): 8 n4 (min(max_iter, N) + 3 + k') bytes for the
 * basis, the two work vectors and the Ritz panel, 8 N k for its product, and 8 (min(max_iter, N) (k + 2)) for coefficients.
 * Checked in this order -- GENPHI_ERR_ARG: NULL plan; k outside [1, min(GENPHI_EIGEN_MAX_K, N)]; tol negative or NaN; max_iter
 * outside [k, 4096]; ldv < k; a Float64 result (GENPHI_FLAG_STORAGE_F64).  GENPHI_ERR_DEVICE: no resident result.  GENPHI_ERR_ARG:
 * fewer than N rows resident (a shard cannot iterate; an empty shard too); NULL values or vectors.  GENPHI_ERR_ALLOC: the scratch
 * block does not fit (the message states the bytes).  After any error the plan stays usable, the resident result is untouched and
 * no output is written.  The call adds nothing to genphi_stats.                                                                  */
#define GENPHI_EIGEN_MAX_K 64
int genphi_result_eigen(genphi_plan *plan, int32_t k, int32_t center, double tol, int32_t max_iter, uint64_t seed,
                        double *values, double *vectors, int64_t ldv, double *residual, int32_t *converged, int32_t *products);

/* The distribution of the pairwise kinships of the resident result, without moving the matrix: the histogram of Phi
 * over all pairs, within and between groups of probands -- the figure that a mean kinship summarises -- in one read of the upper
 * triangle.  Neither GENLIB nor the reference has such a function, so this text is the definition.  N is the number of probands
 * after duplicates collapse (genphi_plan_create).
 *   the pairs         those of genphi_result_over: (i, j) with i in the resident rows [row_begin, row_begin + n_rows), i < j < N; each
 *                     unordered pair once, never the diagonal, never a padding column of the row pitch
 *   edges             n_edges strictly increasing doubles, none NaN; -infinity and +infinity are allowed.  2 <= n_edges <=
 *                     GENPHI_HIST_MAX_EDGES; n_bins = n_edges - 1
 *   bins              a pair counts with x = (double)Phi[i][j]: in bin b when edges[b] <= x < edges[b + 1]; the last bin also holds
 *                     x == edges[n_bins] (numpy.histogram's rule); in `below` when x < edges[0]; in `above` when x > edges[n_bins].
 *                     (An entry is a Float32, so the library compares it with the smallest Float32 at or above each edge -- above the
 *                     last one: for every double edge that decides exactly as the Float64 comparison does, csrc/hist_geometry.h.)
 *   group == NULL     n_groups must be 0 or 1; counts holds n_bins entries, below and above one each
 *   group != NULL     labels as for genphi_result_group_sums: N entries, 0 .. n_groups - 1, or -1 = in no group; 1 <= n_groups <=
 *                     GENPHI_HIST_MAX_GROUPS.  counts is n_groups x n_groups x n_bins, row-major, and SYMMETRIC: counts[a][b][.]
 *                     counts the unordered pairs {i, j}, i resident and i < j, with one member in a and the other in b;
 *                     counts[a][a][.] are the pairs within a.  below and above are n_groups x n_groups, symmetric too.  A pair with
 *                     an unlabelled member counts nowhere.
 *   cells             max(n_groups, 1) x n_bins <= GENPHI_HIST_MAX_CELLS: a workgroup's table of Int32 counters in LDS (64 KB)
 *   *n_pairs          the pairs counted: the sum of bins + below + above over a <= b
 * Any output pointer may be NULL.  Counts are integers, accumulated by integer additions only: the answer is a function of the matrix,
 * the resident rows, the edges and the labels, and the same call gives the same bytes whatever the launch geometry.  The outputs of
 * row shards add.  An empty shard (no resident row after a genphi_compute_device call), or N < 2, is GENPHI_OK with zeros.
 * Device memory, in the plan's scratch block, kept between calls: 4 bytes per resident row, 4 per proband when there are labels,
 * 4 per edge, and 8 max(n_groups, 1)^2 (n_bins + 2) for the table.  The phiOver counts the library keeps (genphi_result_over) are
 * not touched.
 * GENPHI_ERR_ARG: NULL plan or edges, n_edges out of range, edges not strictly increasing or NaN, n_groups out of range, too many
 * cells, a label outside [-1, n_groups), a Float64 result (GENPHI_FLAG_STORAGE_F64); GENPHI_ERR_DEVICE: no resident result;
 * GENPHI_ERR_ALLOC: the scratch does not fit (found before the launch).  After any error the plan stays usable, the resident
 * result is untouched and no output is written.                                                                                   */
#define GENPHI_HIST_MAX_EDGES 4097
#define GENPHI_HIST_MAX_GROUPS 256
#define GENPHI_HIST_MAX_CELLS 16384
int genphi_result_hist(genphi_plan *plan, int32_t n_edges, const double *edges, int32_t n_groups, const int32_t *group,
                       int64_t *counts, int64_t *below, int64_t *above, int64_t *n_pairs);

/* Exact order statistics of the same pairs: the median and the upper quantiles that a genphi_result_over threshold
 * is chosen from, in a few reads of the upper triangle.
 *   values[r]         the entry of 0-based rank ranks[r] among the pairs of the resident rows, sorted ascending: bit for bit an
 *                     entry of the matrix.  Ranks may repeat and come in any order; each lies in [0, *n_pairs).
 *   n_ranks           1 .. GENPHI_SELECT_MAX_RANKS; n_ranks == 0 with values == NULL only reports *n_pairs (ranks is not read)
 *   *n_pairs          the pairs of the resident rows (may be NULL): the sum of N - 1 - i over them
 *   the method        every entry a sweep produces is finite and >= +0, so its unsigned bit pattern orders like its value.  The
 *                     selection is a most-significant-digit radix selection on the patterns: each pass is a histogram of one digit
 *                     of the entries whose higher bits match one of the (distinct) prefixes still alive, and the host narrows
 *                     every rank between passes.  The answer does not depend on the digit width (8 bits: 4 passes, each one read).
 *   row shards        on a shard the answer is over that shard's pairs only.  Order statistics of shards do NOT compose: combine
 *                     the histograms of the shards instead, or select on the full result.
 * An empty shard or N < 2 has no pair: *n_pairs = 0 and every rank is out of range.  Device memory: 4 bytes per resident row and
 * 32 KB of digit tables, in the plan's scratch block.  The same call gives the same bytes.
 * GENPHI_ERR_ARG: NULL plan, n_ranks outside [0, GENPHI_SELECT_MAX_RANKS] or 0 with values given, NULL ranks or NULL values with
 * n_ranks > 0, a rank outside [0, *n_pairs), a Float64 result; GENPHI_ERR_DEVICE: no resident result; GENPHI_ERR_ALLOC: the scratch
 * does not fit (found before the first launch).  After any error the plan stays usable, the resident result is untouched and no
 * output is written.                                                                                                              */
#define GENPHI_SELECT_MAX_RANKS 16
int genphi_result_select(genphi_plan *plan, int32_t n_ranks, const int64_t *ranks, float *values, int64_t *n_pairs);

/* Families and unrelated sets: two questions about the graph G_t whose vertices are the probands and whose edges are the
 * pairs related at or above a threshold t, answered from the resident result in a few passes; the edge list never exists.  Neither
 * GENLIB nor the reference has such functions, so this text is the definition.  N is the number of probands after duplicates collapse
 * (genphi_plan_create); positions are 0-based in that order.
 *   edge rule         positions i != j are joined iff (double)Phi[i][j] >= threshold: the rule of genphi_result_over
 *   padding           the padding columns j >= N of the row pitch hold zeros and are never edges: a threshold <= 0 does not join them
 *   diagonal          never an edge
 *   threshold         any double but NaN; +infinity gives no edge, -infinity joins every pair
 *   the full result   both calls need the full Float32 result resident (row_begin == 0, n_rows == N): a row shard (an empty one too) is
 *                     GENPHI_ERR_ARG, a Float64 result (GENPHI_FLAG_STORAGE_F64) is GENPHI_ERR_ARG, a plan without a resident result
 *                     is GENPHI_ERR_DEVICE.  N = 0 or N = 1 is GENPHI_OK with the trivial answer (checked before the result is).
 *   after an error    the plan stays usable, the resident result is untouched, and no output is written
 *
 * genphi_result_clusters: the connected components of G_t.
 *   label[i]          the smallest position in i's component: label[i] <= i and label[label[i]] == label[i]
 *   *n_clusters       the positions with label[i] == i
 *   *n_pairs          the edges i < j: the count of the count-only call of genphi_result_over at the same threshold
 * Any output pointer may be NULL.  One read of the upper triangle (2 N^2 bytes) by a lock-free union-find, then a pass over N entries.
 * The answer is a function of the matrix and the threshold alone, whatever the order in which the device meets the edges.  Device
 * memory, in the plan's scratch block: 8 N bytes (a parent and a per-row edge count for every proband).
 *
 * genphi_result_unrelated: a maximal set of probands no two of which are joined -- the "kinship cutoff" of association studies.
 *   degree[i]         the edges at i
 *   the order         vertices are visited in ascending order of the key (priority[i], i); priority == NULL means the key
 *                     (degree[i], i): the fewest relatives first, the usual heuristic for a large set
 *   member[i]         1 or 0: the answer of the sequential greedy rule -- visit the vertices in that order and take a vertex iff none
 *                     of its neighbours has been taken.  The answer is unique: a function of the matrix, the threshold and the
 *                     priorities alone.  It is a maximal independent set of G_t.
 *   *n_members        the members
 *   *rounds           the launches of the round kernel: diagnostic, not part of the answer (it may differ from call to call)
 * member may not be NULL (GENPHI_ERR_ARG); the other outputs may be.  One full read of the matrix (4 N^2 bytes) for the degrees -- left out
 * when priorities are given and degree is NULL -- then rounds: a launch reads the rows of the vertices still undecided, 4 N bytes each
 * (less where a member is met early), and the host reads one 8-byte count after it.  At most N rounds; a graph that is one long path
 * visited from one end needs about N / 2, each over two rows.  Device memory, in the plan's scratch block: 13 N bytes (a state byte, a
 * 64-bit key and a degree for every proband).
 *
 * The phiOver counts the library keeps (genphi_result_over) are not touched by either call.
 * GENPHI_ERR_ARG: NULL plan, NaN threshold, NULL member, a Float64 result, a row shard; GENPHI_ERR_DEVICE: no resident result;
 * GENPHI_ERR_ALLOC: the scratch does not fit (found before the first launch).                                                       */
int genphi_result_clusters(genphi_plan *plan, double threshold, int32_t *label, int64_t *n_clusters, int64_t *n_pairs);
int genphi_result_unrelated(genphi_plan *plan, double threshold, const int32_t *priority, uint8_t *member, int32_t *degree,
                            int64_t *n_members, int32_t *rounds);

/* The single-linkage tree of the kinships: which probands merge at which kinship, from the closest pairs down to `floor`.
 * It is the maximum spanning forest of the graph of genphi_result_clusters taken at every threshold at once, found on the resident
 * result by Boruvka's rounds.  Neither GENLIB nor the reference has such a function, so this text is the definition.  N is the number
 * of probands after duplicates collapse (genphi_plan_create); positions are 0-based in that order.
 *   edges             the pairs i < j with (double)Phi[i][j] >= floor: the rule and the comparison of genphi_result_over.  floor <= 0
 *                     makes every pair an edge, +infinity gives no edge, NaN is an error.  The padding columns j >= N of the row pitch
 *                     never take part, and neither does the diagonal.
 *   the order         edge (i, j) precedes (i', j') when its kinship is larger, then when i is smaller, then when j is smaller.
 *                     Entries are finite and >= +0, so the Float32 bit pattern orders like the value: a strict total order.
 *   the forest        an edge belongs to the forest iff no path of preceding edges joins its ends (Kruskal's rule).  Under a strict
 *                     order the forest is unique: a function of the matrix and floor alone.
 *   row, col, kinship the M = N - *n_trees edges of the forest in that order: row[k] < col[k], kinship[k] the entry Phi[row[k]][col[k]]
 *                     bit for bit.  The caller gives arrays of N - 1 entries; entries from M on are not written.
 *   *n_edges          M
 *   *n_trees          the connected components of the graph at `floor`: the n_clusters of genphi_result_clusters(floor)
 *   *rounds           the rounds it took; the number genphi_tree_host takes on the same matrix
 * Any output pointer may be NULL.  Invariants:
 *   1. for every t >= floor the connected components of the listed edges with kinship >= t are exactly the labels of
 *      genphi_result_clusters(t);
 *   2. the number of listed edges with kinship >= t is N - n_clusters(t);
 *   3. a larger floor gives the prefix of the list that passes it;
 *   4. the same call gives the same bytes;
 *   5. *rounds <= ceil(log2 N) + 1, and it equals the host restatement's.
 * A round: every row of a component that still grows is read whole (4 N bytes; the best edge out of a component may lead to a column
 * left of the row) for the row's best edge out of its component; every component picks the best of its rows' edges under the order
 * above, by integer atomic maxima and minima only; the picked edges, each once, go to the forest and join their ends (the lock-free
 * union-find of genphi_result_clusters); the labels are flattened, and the host reads 8 bytes: the edges of the round.  A component
 * that finds no edge out is a finished tree and its rows are not read again.  It ends after a round without an edge or when N - 1
 * edges are there; a round with an edge at least halves the components that still grow.  The list is sorted on the host.
 * The full Float32 result must be resident, as for genphi_result_clusters: a row shard (an empty one too) is GENPHI_ERR_ARG, a Float64
 * result is GENPHI_ERR_ARG, a plan without a resident result GENPHI_ERR_DEVICE; N = 0 or N = 1 is GENPHI_OK with no edge, N trees and
 * 0 rounds (checked before the result is).  Device memory, in the plan's scratch block: 41 N bytes (per proband two labels, an 8-byte
 * row key, a 4-byte and an 8-byte component key, a flag, and a 12-byte slot of the edge buffer).  The phiOver counts the library keeps
 * are not touched.  GENPHI_ERR_ARG: NULL plan, NaN floor, a Float64 result, a row shard; GENPHI_ERR_DEVICE: no resident result;
 * GENPHI_ERR_ALLOC: the scratch does not fit (found before the first launch).  After an error the plan stays usable, the resident
 * result is untouched, and no output is written.
 *
 * genphi_tree_host: host only (no GPU), in the role of genphi_link_words: the same rounds with the same key arithmetic (csrc/tree_keys.h)
 * on a host matrix m of n rows with row pitch ld >= n (the columns from n on are never read).  m must be symmetric with finite entries
 * >= +0, as a result is; both halves are read, as on the device.  The same outputs; GENPHI_ERR_ARG: n outside [0, 2^31), NaN floor,
 * NULL m with n >= 2, ld < n.                                                                                                       */
int genphi_result_tree(genphi_plan *plan, double floor, int32_t *row, int32_t *col, float *kinship, int64_t *n_edges, int64_t *n_trees,
                       int32_t *rounds);
int genphi_tree_host(const float *m, int64_t n, int64_t ld, double floor, int32_t *row, int32_t *col, float *kinship, int64_t *n_edges,
                     int64_t *n_trees, int32_t *rounds);

/* GENLIB's gen.phiCI(phiMatrix, prob, b) and gen.fCI(vectF, prob, b): bootstrap confidence intervals of the mean kinship and of the
 * mean inbreeding.  The reference has neither, so this text is the definition.  N is the number of probands after
 * duplicates collapse (genphi_plan_create), N >= 2.
 *   the draws         resample r >= 0 draws the N probands N times with replacement.  Draw k in [0, N): one Philox4x32-10 block (the
 *                     generator of genphi_simu_*, below) with counter (k >> 1, r, 0, 2) and key (seed low 32, seed high 32) gives
 *                     the words W0 = o0 | o1 << 32 and W1 = o2 | o3 << 32; draw k uses W_(k & 1); the drawn position is
 *                     s = (W * N) >> 64, the high half of the 128-bit product.  The fourth counter word 2 keeps these blocks apart
 *                     from gene dropping's (0 and 1 there).  c_r[i] = the number of draws of resample r that gave i.  The counts are a
 *                     pure function of (N, seed, r): not of b, of how resamples are grouped into panels, or of the resident rows.
 *                     Known answers (N, seed, r, k -> s): 140, 0, 0, 0 -> 95;  140, 0, 0, 1 -> 115;
 *                     100000, 0x123456789abcdef, 4999, 99999 -> 67714.
 *   the statistic     theta_r = (sum_i sum_j c_r[i] c_r[j] Phi[i][j] - sum_i c_r[i] Phi[i][i]) / (N (N - 1)): phiMean
 *                     (src/compute.jl:454-459) of the resampled matrix Phi[s, s].  A proband drawn twice puts its self-kinship at two
 *                     off-diagonal positions of that matrix; those stay in.  For gen.fCI: theta_r = sum_i c_r[i] F[i] / N.
 *   the interval      quantiles of theta_0 .. theta_(b-1) by linear interpolation of the sorted values (R's type 7, numpy.quantile's
 *                     default), taken by the caller.
 * genphi_bootstrap_counts: host only (no GPU).  counts[n_boot][n] (row-major) receives c_r for r = first .. first + n_boot - 1.
 *   GENPHI_ERR_ARG: n outside [2, 2^31), n_boot < 1, first < 0, first + n_boot >= 2^31, counts NULL.
 * genphi_result_bootstrap: on the resident Float32 result, without moving the matrix.  For r = first .. first + n_boot - 1:
 *   quad[r - first]   sum over the resident rows i and all columns j < N of c_r[i] c_r[j] Phi[i][j]
 *   self[r - first]   sum over the resident rows i of c_r[i] Phi[i][i]
 *   *n_rows           the resident rows (may be NULL; quad and self may be NULL too)
 *                     Both are additive over row shards, as genphi_result_sums is; theta_r = (quad - self) / (N (N - 1)) of the sums.
 *                     `first` lets a caller split the resamples over calls: first = 37, n_boot = 20 gives entries 37 .. 56 of
 *                     first = 0, n_boot = 64, bit for bit.
 *   arithmetic        Float64 throughout: c_j Phi[i][j] is exact, accumulation is by fma in a fixed order (no floating-point
 *                     atomics), so the same call returns the same bits.  All terms are >= 0: quad is within 3 n_rows N 2^-53
 *                     relative of the exact sum, self within n_rows 2^-53; where every entry of Phi is a multiple of 2^-k and
 *                     N^2 max(c)^2 2^k < 2^53 both are exact.
 *   panels            resamples are worked off in panels (GENPHI_BOOT_PANEL; default: what keeps a panel's Int32 counts, 4 bytes per
 *                     proband and resample, within 256 MiB, at least 128, at most 8192): counts on the device, then the product of
 *                     the resident rows with the panel fused with its reduction, then a reduction of the row blocks' partials.
 *                     Device memory: the counts of a panel, 16 bytes per (block of 128 resident rows, resample of a panel) and
 *                     16 bytes per resample, in the plan's scratch block, kept between calls.  Work: 2 n_rows N n_boot Float64
 *                     operations; symmetry is not used.
 * An empty shard (no resident row after a genphi_compute_device call) is GENPHI_OK with zeros.
 * GENPHI_ERR_ARG: NULL plan, n_boot < 1, first < 0, first + n_boot >= 2^31, N < 2, a Float64 result (GENPHI_FLAG_STORAGE_F64);
 * GENPHI_ERR_DEVICE: no resident result; GENPHI_ERR_ALLOC: the scratch block does not fit in device memory (found before any
 * launch).  After any error the plan stays usable and the resident result is untouched.                                         */
int genphi_bootstrap_counts(int64_t n, uint64_t seed, int32_t first, int32_t n_boot, int32_t *counts);
int genphi_result_bootstrap(genphi_plan *plan, uint64_t seed, int32_t first, int32_t n_boot, double *quad, double *self,
                            int64_t *n_rows);

/* Point lookups in the resident result without moving the matrix: out[k] = Phi[rows[k], cols[k]]
 * (0-based positions in proband order, duplicates collapsed as in genphi_plan_create; rows must
 * lie in the resident row range).  This is what gen.f(pedigree, IDs) (src/compute.jl:500-511)
 * needs: the inbreeding coefficient of x is the kinship of its parents, one entry of the sweep
 * over the parents instead of the reference's un-memoised pairwise recursion (:66-95).  Values
 * are the Float32 entries widened to Float64.                                                  */
int genphi_result_entries(genphi_plan *plan, int64_t n, const int64_t *rows, const int64_t *cols,
                          double *out);

/* Convenience = genphi_compute_device + genphi_result_to_host: what the Julia shim's
 * phi(...; compute=true) calls.  out: N x N Float32, caller-owned.                           */
int genphi_compute_f32(genphi_plan *plan, float *out, const genphi_opts *opts,
                       genphi_stats *stats);

/* Native loader for the step before the path: gen.genealogy(filename; sort) (src/create.jl:161-189:
 * header row skipped, four whitespace-separated integers `ind father mother sex` per row) plus,
 * with sort != 0, _ordered_pedigree (src/create.jl:196-227: stable sort by maximum ancestral
 * depth).  Returns the pedigree in RANK ORDER, ready for genphi_plan_create, in arrays
 * allocated by the library (release each with genphi_free).  sex_out may be NULL.  Unknown
 * parent -> GENPHI_ERR_UNKNOWN_ID; sort == 0 and a parent after its child -> GENPHI_ERR_ORDER. */
int genphi_genealogy_read(const char *path, int32_t sort, int64_t *n, int64_t **ind, int64_t **father,
                          int64_t **mother, int64_t **sex_out);
/* The same for a table already in memory (gen.genealogy(dataframe; sort), src/create.jl:131-146, ordered by :196-254): ind / father /
 * mother (/ sex, may be NULL) in file order -> malloc'ed arrays in rank order (release with genphi_free).  Errors as
 * genphi_genealogy_read: GENPHI_ERR_DUPLICATE_ID, GENPHI_ERR_UNKNOWN_ID (a parent that is not an individual: KeyError in the reference),
 * GENPHI_ERR_ARG (a cycle), and with sort = 0 GENPHI_ERR_ORDER (a parent listed after its child: KeyError, src/create.jl:240-241). */
int genphi_genealogy_order(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, const int64_t *sex,
                           int32_t sort, int64_t *n_out, int64_t **ind_out, int64_t **father_out, int64_t **mother_out,
                           int64_t **sex_out);
void genphi_free(void *ptr);

/* gen.branching(pedigree; pro, ancestors) (src/extract.jl:65-186), the pruning step before the
 * path: keeps the individuals on the paths between the selected probands and ancestors.
 * Input: the pedigree in rank order (as for genphi_plan_create) plus sex (may be NULL -> 0).
 * pro == NULL / ancestors == NULL mean "not given" (Julia `nothing`): with only pro, the
 * probands and all their ancestors are kept; with only ancestors, they and all their
 * descendants (parents outside the set become unknown); with both, the intersection (parents
 * outside it become unknown); with neither, nobody.  Output arrays are in the input's rank
 * order, allocated by the library (genphi_free each).  Unknown ID -> GENPHI_ERR_UNKNOWN_ID.   */
int genphi_branching(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                     const int64_t *sex, int64_t n_pro, const int64_t *pro, int64_t n_anc,
                     const int64_t *ancestors, int64_t *n_out, int64_t **ind_out, int64_t **father_out,
                     int64_t **mother_out, int64_t **sex_out);

/* What the library keeps between calls, per process: device blocks of released plans (up to GENPHI_KEEP_MB, default 8 GiB but at most 1/16 of the device's memory, per
 * device, handed to the next plan instead of hipMalloc / hipFree), idle streams, the pinned staging ring of genphi_result_to_host,
 * and the device side + pinned buffer of the last genphi_sparse_phi call (up to GENPHI_SPARSE_KEEP_MB, default 1024).  A one-shot
 * gen.phi call on a mid-size pedigree otherwise spends most of its time in the allocator.  genphi_release_cached gives all of it
 * back to the driver (plans in use are not touched); genphi_cached_bytes = device bytes kept right now.  The reference has no
 * counterpart: its matrices are garbage-collected Julia arrays (src/compute.jl:291,301).                                      */
void genphi_release_cached(void);
int64_t genphi_cached_bytes(void);

/* Releases everything the plan holds on its GPU (index arrays, level matrices, the resident
 * result, streams, captured graphs) and keeps the host-side plan: the next genphi_compute_device
 * uploads again, on the same or on another device (opts->device).  The reference has no
 * counterpart (its matrices are garbage-collected Julia arrays, src/compute.jl:291,301).      */
int genphi_plan_release_device(genphi_plan *plan);

/* ---- gen.sparse_phi / KinshipMatrix (src/compute.jl:321-447, :31-46, :467-472) -------------------
 * The reference's second kinship algorithm: individuals are processed one at a time in queue order,
 * each kinship is RN32(phi[father, j]/2 + phi[mother, j]/2), parents are dropped when their children
 * are done, and the result is a dictionary of the probands' non-zero kinships keyed by rank.  Here the
 * queue is simulated on the host (integers only) and all individuals of one depth are computed by two
 * streaming kernels on a dense "active" matrix in HBM (csrc/sparse_phi.hip).  Values, getindex
 * semantics (incl. the reference's (earlier, later) vs (smaller, larger rank) key behaviour), the
 * number of stored entries `show` prints and phiMean's sums are those of the reference.
 *   genphi_sparse_phi      sparse_phi(pedigree, probandIDs); pedigree in rank order as for
 *                          genphi_plan_create; runs on the GPU (no CPU fallback)
 *   genphi_sparse_info     n_rows x n_rows KinshipMatrix with n_stored entries; Float64 sums of all
 *                          stored values and of the self kinships (phiMean = (all - diag) / (n (n-1) / 2))
 *   genphi_sparse_get      getindex(phi, ID1, ID2) for n pairs; an ID that is not a proband ->
 *                          GENPHI_ERR_UNKNOWN_ID (KeyError in the reference)
 *   genphi_sparse_entries  every stored entry as (row rank, column rank, value); returns their number
 *                          (the arrays may be NULL / cap 0 to ask for it)                               */
typedef struct genphi_sparse genphi_sparse;
int genphi_sparse_phi(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                      int64_t n_pro, const int64_t *pro_ids, int32_t device, genphi_sparse **out);
int genphi_sparse_info(const genphi_sparse *h, int64_t *n_rows, int64_t *n_stored, double *sum_all, double *sum_diag);
/* Measurement of the sweep that built the handle: number of waves (depths), device time of the sweep and of each
 * wave (HIP events on its stream; the first `cap` waves), algorithmic bytes 4 (n_old^2 + n_next^2) per wave (the
 * active matrix read once, the next one written once) and in total, the largest active set.  Any pointer may be NULL. */
int genphi_sparse_stats(const genphi_sparse *h, int32_t *n_waves, double *sweep_ms, double *algorithmic_bytes,
                        int64_t *max_active, float *wave_ms, double *wave_bytes, int32_t cap);
/* Host only, no GPU needed (diagnostic, no reference counterpart as a function): the schedule genphi_sparse_phi follows -- the order
 * in which individuals leave the reference's queue (src/compute.jl:336-345 founders, :431-439 children) as IDs, for each the processing
 * index at which it is dropped from the live set (:401-430: when its last child is processed; -1 = a proband, never dropped) and its
 * wave (one wave per depth).  *n_out = the number of individuals processed (the probands and their ancestors); at most `cap` entries
 * of each array that is not NULL are filled.  Errors as genphi_sparse_phi (unknown proband, parent after child, duplicate ID). */
int genphi_sparse_schedule(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                           const int64_t *pro_ids, int64_t cap, int64_t *order_ids, int64_t *retire_at, int32_t *wave, int64_t *n_out);
int genphi_sparse_get(const genphi_sparse *h, int64_t n, const int64_t *id1, const int64_t *id2, double *out);
int64_t genphi_sparse_entries(const genphi_sparse *h, int64_t cap, int64_t *row_rank, int64_t *col_rank, float *val);
void genphi_sparse_destroy(genphi_sparse *h);

/* ---- storage-sharded gen.phi: column panels + an exchange step (csrc/panel_phi.hip) --------------------
 * For pedigrees whose level matrices do not fit one GPU (the reference keeps two dense level matrices
 * alive, src/compute.jl:291,301).  Rank r of `world` stores the column panel of the members it owns (all
 * rows x its columns: 1/world of every level matrix) and, before every level step, receives the parent
 * columns of its new members that other ranks own.  This library packs / consumes DEVICE buffers; the
 * all-to-all itself is issued by the host (torch.distributed over RCCL/xGMI: genlib.jl_amd/distributed.py).
 *   create            plan + ownership + exchange lists (host only; identical arguments on every rank)
 *   begin             upload, Psi_1 = 1/2 I on the local columns
 *   exchange_counts   columns to send to / receive from every rank before step `step`, floats per column
 *   pack / compute    fill the send buffer; unpack the received columns and run the level step: the FULL / SPLIT
 *                     row kernels of the dense path on this rank's local columns (source rows = rows of the
 *                     rank's extended panel), the per-entry kernel when a panel row does not fit in LDS
 *   result_to_host    this rank's row block [row_begin, row_begin + n_rows) of Phi (proband order)      */
typedef struct genphi_panel genphi_panel;
int genphi_panel_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                        int64_t n_pro, const int64_t *pro_ids, int32_t rank, int32_t world, genphi_panel **out);
int64_t genphi_panel_n_steps(const genphi_panel *p);
double genphi_panel_step_ms(const genphi_panel *p, int32_t step);  /* device time of the step's kernels (unpack + level) in the last sweep, HIP events; -1 bad argument */
int genphi_panel_step_mode(const genphi_panel *p, int32_t step);   /* 0 FULL / 1 SPLIT row kernels on the local columns, 2 per-entry kernel; -1 bad argument */
int64_t genphi_panel_n_probands(const genphi_panel *p);
int genphi_panel_result_rows(const genphi_panel *p, int64_t *row_begin, int64_t *n_rows);
int genphi_panel_exchange_counts(const genphi_panel *p, int32_t step, int64_t *send_cols, int64_t *recv_cols, int64_t *col_floats);
double genphi_panel_device_bytes(const genphi_panel *p);
int genphi_panel_begin(genphi_panel *p, int32_t device);
int genphi_panel_pack(genphi_panel *p, int32_t step, float *d_send);
int genphi_panel_compute(genphi_panel *p, int32_t step, const float *d_recv);
/* The same two calls ordered by streams instead of host synchronisations (what distributed.py uses): caller_stream is the
 * hipStream_t the host driver enqueues its collective on (torch's current stream).  pack_on makes caller_stream wait for the
 * packed columns; compute_on makes the panel's stream wait for what caller_stream holds (the collective) before it unpacks.
 * Neither blocks the host; genphi_panel_sync (or result_to_host / step_ms) waits for the sweep.  caller_stream =
 * GENPHI_NO_STREAM: no collective runs between the two calls (a single rank), nothing is ordered across streams.        */
#define GENPHI_NO_STREAM ((void *)(intptr_t)-1)
int genphi_panel_pack_on(genphi_panel *p, int32_t step, float *d_send, void *caller_stream);
int genphi_panel_compute_on(genphi_panel *p, int32_t step, const float *d_recv, void *caller_stream);
int genphi_panel_sync(genphi_panel *p);
int genphi_panel_result_to_host(genphi_panel *p, float *out);
void genphi_panel_destroy(genphi_panel *p);

/* ---- gen.gc: genetic contributions of ancestors to probands (csrc/gc.hip) -----------------------------------
 * Replaces gc(pedigree; pro = pro(pedigree), ancestors = founder(pedigree)), src/compute.jl:518-595 (GENLIB's Congen).
 * Result: Float32, n_pro x n_anc, row-major (ld = n_anc), rows in pro_ids order, columns in anc_ids order (a Julia
 * Matrix{Float32}(undef, n_anc, n_pro) receives its transpose).  Entry [i][j] = sum over every descending path from
 * anc_ids[j] to pro_ids[i] of 0.5^length.  The reference's rules, kept here:
 *   - only LEAVES (individuals with no children anywhere in the pedigree) receive contributions: a proband with
 *     children gets a row of zeros;
 *   - the reference reads and resets a proband's accumulator after each ancestor, so a proband ID listed again gets a
 *     row of zeros: only its first occurrence carries values;
 *   - a duplicated ancestor gives identical columns; an ancestor that is itself a leaf proband gets 1 on its own row;
 *     an ancestor with parents is allowed (its parents add nothing to its column); an ancestor with no path to a
 *     proband gives a zero column; an unknown ID in pro_ids or anc_ids -> GENPHI_ERR_UNKNOWN_ID (KeyError);
 *   - n_pro = 0 or n_anc = 0: an empty result of that shape.
 * Exactness.  The sweep runs over the planner's generation cuts; after c steps every value is a multiple of 2^-c in
 * [0, 1], and the rows are kept in Float64 and rounded to Float32 once.  So the result is the exact contribution
 * correctly rounded to Float32 for sweeps of up to 52 steps, and within 1 Float32 ulp of it beyond (normal range).  The
 * reference adds paths one at a time in Float32: its sums are exact, and equal to this result bit for bit, while the
 * sweep has at most 24 steps (geneaJi, genea140, cfg3); deeper, its own rounding depends on the order of its paths and
 * may differ from the correctly rounded value returned here.
 *   create            host only (no GPU): checks IDs and pedigree order, plans cuts, rows and slots
 *   compute           the sweep on `device` (-1 = current); the result stays resident on the device; GENPHI_ERR_ALLOC
 *                     before any launch when the result or the slot rows do not fit
 *   result_device     device pointer and row pitch (floats) of the resident result
 *   result_to_host    out: n_pro x n_anc Float32, row-major
 *   stats             device time of the last sweep (HIP events), its algorithmic bytes (source rows read and rows
 *                     written at 8 bytes per column, plus the 4-byte result), the slot rows of one panel, the panel width */
typedef struct genphi_gc genphi_gc;
int genphi_gc_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                     int64_t n_pro, const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, genphi_gc **out);
int genphi_gc_compute(genphi_gc *h, int32_t device);
int genphi_gc_result_device(const genphi_gc *h, const float **d_ptr, int64_t *ld);
int genphi_gc_result_to_host(genphi_gc *h, float *out);
int genphi_gc_stats(const genphi_gc *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *panel_cols);
void genphi_gc_destroy(genphi_gc *h);

/* ---- gen.occ and gen.rec: occurrences and coverage of ancestors (csrc/occ.hip) ---------------------------------
 * Replace occ(pedigree; pro = pro(pedigree), ancestors = founder(pedigree), typeOcc = "IND"), src/describe.jl:184-238, and
 * rec(pedigree, probandIDs = pro(pedigree), ancestorIDs = founder(pedigree)), src/describe.jl:133-145.  Both run on the host
 * schedule of gen.gc (csrc/ancestor_sweep.h): generation cuts, slot rows, column panels sized for the Infinity Cache.
 *
 * occ.  Entry [i][j] = the number of ascending paths from pro_ids[i] to anc_ids[j], by the recursion
 * N[x] = N[father] + N[mother], then N[x][j] += 1 where anc_ids[j] == x.  Result: Int64, n_pro x n_anc, row-major
 * (ld = n_anc), rows in pro_ids order, columns in anc_ids order: exactly the memory of the reference's
 * Matrix{Int}(undef, n_anc, n_pro), which wraps it without a transpose.  The reference's rules, kept here:
 *   - every proband carries values, with or without children; a proband listed again gets the same row again;
 *   - a proband that is itself a requested ancestor counts the path of length 0 (1 on that entry);
 *   - an ancestor with parents is allowed; its own ancestors may be requested too (paths run through it);
 *   - a duplicated ancestor ID: only its FIRST column carries values, later ones are zero (the reference reads and resets
 *     the ancestor's counter row by row) -- the opposite of gen.gc;
 *   - an unknown ID in pro_ids or anc_ids -> GENPHI_ERR_UNKNOWN_ID (KeyError); n_pro = 0 or n_anc = 0: an empty result.
 * Exactness.  Rows are unsigned 64-bit integers added with wrap-around.  Addition modulo 2^64 commutes with the recursion
 * and the reference's Int wraps the same way, so the result equals the reference's bit for bit at any depth, read as Int64
 * (2^63 paths read -2^63, 2^64 paths read 0).  In cut c every count is at most 2^c, so sweeps of at most 31 steps run on
 * unsigned 32-bit slot rows (half the bytes, the same Int64 result) unless GENPHI_OCC_ROWS64 is given.
 * TOTAL (the reference's sum(occ, dims = 2); a proband listed k times counts k times): a handle created with
 * GENPHI_OCC_TOTAL_ONLY reduces the last step on the device into n_anc Int64 totals (per-row-group partial sums, then 64-bit
 * integer atomics: the same bits on every run) and never allocates an n_pro x n_anc buffer.
 *   create            host only (no GPU): checks IDs and pedigree order, plans cuts, rows and slots
 *   compute           the sweep on `device` (-1 = current); the result stays resident; GENPHI_ERR_ALLOC before any launch
 *                     when the result or the slot rows do not fit
 *   result_device     device pointer and row pitch (Int64 entries) of the resident result (GENPHI_ERR_ARG on a TOTAL-only handle)
 *   result_to_host    out: n_pro x n_anc Int64, row-major (GENPHI_ERR_ARG on a TOTAL-only handle)
 *   totals            out: n_anc Int64; on a handle with a full result, its column sums taken on the device
 *   stats             device time of the last sweep (HIP events), its algorithmic bytes (source rows read and rows written
 *                     at the row width per panel column, plus the 8-byte result entries or totals), the slot rows of one
 *                     panel, the panel width, the row width in bits (64 or 32) and the kernel launches of the sweep
 *
 * rec.  Entry [j] = the number of distinct pro_ids that descend from anc_ids[j], by the recursion R[x] = R[father] | R[mother],
 * then R[x][j] = 1 where anc_ids[j] == x, on bit rows (64 ancestor columns per 64-bit word), followed by a column count over
 * the probands' rows.  Not derived from occ: a path count can wrap to 0 while the ancestor is still an ancestor.  Rules kept:
 *   - descendants are strict: an ancestor that is itself a proband does not count itself;
 *   - a proband listed twice counts once; a proband ID that is not in the pedigree is ignored;
 *   - a duplicated ancestor gives equal entries; probands with children count like any other;
 *   - an unknown ancestor ID -> GENPHI_ERR_UNKNOWN_ID (KeyError).
 *   result            out: n_anc Int64 (host)
 *   stats             as above; algorithmic bytes at 8 bytes per 64 columns, plus one read of every proband row by the count;
 *                     row width 64                                                                                       */
#define GENPHI_OCC_TOTAL_ONLY 1   /* totals only: no n_pro x n_anc result exists */
#define GENPHI_OCC_ROWS64 2       /* 64-bit slot rows even where 32-bit rows are exact */
typedef struct genphi_occ genphi_occ;
int genphi_occ_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                      int64_t n_pro, const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, int32_t flags, genphi_occ **out);
int genphi_occ_compute(genphi_occ *h, int32_t device);
int genphi_occ_result_device(const genphi_occ *h, const int64_t **d_ptr, int64_t *ld);
int genphi_occ_result_to_host(genphi_occ *h, int64_t *out);
int genphi_occ_totals(genphi_occ *h, int64_t *out);
int genphi_occ_stats(const genphi_occ *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *panel_cols,
                     int32_t *row_bits, int64_t *launches);
void genphi_occ_destroy(genphi_occ *h);
typedef struct genphi_rec genphi_rec;
int genphi_rec_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                      int64_t n_pro, const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, genphi_rec **out);
int genphi_rec_compute(genphi_rec *h, int32_t device);
int genphi_rec_result(genphi_rec *h, int64_t *out);
int genphi_rec_stats(const genphi_rec *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *panel_cols,
                     int32_t *row_bits, int64_t *launches);
void genphi_rec_destroy(genphi_rec *h);

/* ---- gen.meioses, gen.findMRCA: shortest ascents (csrc/dist.hip) and the host glue of the MRCA family (csrc/loader.cpp) -------
 * Replace findMRCA / findDistance / findFounders / ancestor (src/identify.jl:83-199) and _findMinDistance (src/describe.jl:241-289).
 *
 * dist.  Entry [i][j] = the number of meioses on the SHORTEST ascending path from pro_ids[i] to anc_ids[j], by the min-plus
 * recursion D[x] = min(D[father], D[mother]) + 1, then D[x][j] = 0 where anc_ids[j] == x, on the host schedule of gen.gc /
 * gen.occ (csrc/ancestor_sweep.h).  Result: signed 16-bit, n_pro x n_anc, rows in pro_ids order (one row per occurrence), columns
 * in anc_ids order; -1 = anc_ids[j] is neither pro_ids[i] nor one of its ancestors.  Rules:
 *   - every proband gets its row, with or without children; a proband listed again gets the same row again;
 *   - a proband that is itself a requested ancestor is at distance 0 from itself;
 *   - an ancestor with parents is allowed and its own ancestors may be requested too; a duplicated ancestor gives equal columns;
 *   - an unknown ID in pro_ids or anc_ids -> GENPHI_ERR_UNKNOWN_ID (KeyError); n_pro = 0 or n_anc = 0: an empty result.
 * Depth.  A distance is at most the number of level steps of the sweep (generation cuts - 1).  Slot rows are unsigned 16-bit
 * (65535 - distance, 0 = none) and the result is signed: sweeps of up to GENPHI_DIST_MAX_STEPS = 32767 steps are covered, and
 * create returns GENPHI_ERR_ARG for a deeper one instead of wrapping.
 *   create            host only (no GPU): checks IDs, pedigree order and depth, plans cuts, rows and slots
 *   compute           the sweep on `device` (-1 = current); the result stays resident; GENPHI_ERR_ALLOC before any launch when
 *                     the result or the slot rows do not fit
 *   result_device     device pointer and row pitch in entries: ld = n_anc rounded up to a multiple of 8 (rows start on 16
 *                     bytes); the entries [n_anc, ld) of a row are undefined
 *   result_to_host    out: n_pro x n_anc Int16, row-major, packed (ld = n_anc)
 *   stats             device time of the last sweep (HIP events), its algorithmic bytes (source rows read and rows written at 2
 *                     bytes per panel column, plus the 2-byte result entries), the slot rows of one panel, the panel width, the
 *                     row width in bits (16) and the kernel launches of the sweep
 *
 * genphi_ancestors    gen.ancestor: the strict ancestors of ids[0 .. n_ids) (the union over them), ascending; *out is allocated by
 *                     the library (genphi_free).  Host only.  Unknown ID -> GENPHI_ERR_UNKNOWN_ID.
 * genphi_mrca_filter  of the common ancestors of a group (the full intersection of their ancestor sets), those without a common
 *                     child: the reference's setdiff(common, ancestor(common)) in one pass over the parent arrays.  out: room for
 *                     n_common IDs; the kept IDs in the order given.  Host only.                                             */
#define GENPHI_DIST_MAX_STEPS 32767
typedef struct genphi_dist genphi_dist;
int genphi_dist_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                       int64_t n_pro, const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, genphi_dist **out);
int genphi_dist_compute(genphi_dist *h, int32_t device);
int genphi_dist_result_device(const genphi_dist *h, const int16_t **d_ptr, int64_t *ld);
int genphi_dist_result_to_host(genphi_dist *h, int16_t *out);
int genphi_dist_stats(const genphi_dist *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *panel_cols,
                      int32_t *row_bits, int64_t *launches);
void genphi_dist_destroy(genphi_dist *h);
int genphi_ancestors(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_ids,
                     const int64_t *ids, int64_t *n_out, int64_t **out);
int genphi_mrca_filter(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_common,
                       const int64_t *common, int64_t *n_out, int64_t *out);

/* ---- gen.depths: the number, the shortest, the longest and the mean length of the ascents (csrc/depth.hip) ----------------------
 * Completes _findDistance (src/describe.jl:241-279), which returns the length of every ascending path between a descendant and an
 * ancestor; GENLIB's gen.min / gen.max / gen.mean are its reductions over the founders.
 *
 * depth.  For pro_ids[i] and anc_ids[j], over all ascending paths from the proband to the ancestor (length = meioses; the empty
 * path counts where the proband is the ancestor): paths = their number P, min / max = the shortest / longest length, mean = S / P
 * with S the sum of the lengths.  One exact integer recursion over the generation cuts on the host schedule of gen.gc / gen.occ
 * (csrc/ancestor_sweep.h), on 16-byte elements (csrc/depth_word.h):
 *     P[x] = P[f] + P[m],  S[x] = S[f] + S[m] + P[x],  min[x] = min(min[f], min[m]) + 1,  max[x] = max(max[f], max[m]) + 1,
 * then P = 1, S = 0, min = max = 0 where anc_ids[j] == x.  Without a path: paths 0, mean NaN, min = max = -1.
 *   by = GENPHI_DEPTH_BY_PAIR      n_pro x n_anc entries, rows in pro_ids order (one row per occurrence), columns in anc_ids order
 *   by = GENPHI_DEPTH_BY_PROBAND   n_pro entries: over the paths from pro_ids[i] to ANY listed ancestor (paths and S added, min and
 *                                  max taken over the columns), reduced on the device
 *   by = GENPHI_DEPTH_BY_ANCESTOR  n_anc entries: over the paths from ANY listed proband (each time it is listed) to anc_ids[j],
 *                                  reduced on the device; no n_pro x n_anc buffer exists
 * The reductions add and compare integers only (no floating-point atomics): the same call gives the same bytes whatever the
 * panels, and mean = double(sum S) / double(sum P).  Rules:
 *   - every proband gets its row, with or without children; a proband listed again gets the same row again;
 *   - a proband that is itself a requested ancestor has one path of length 0 to itself (1, 0, 0, 0.0);
 *   - BY_PAIR, BY_ANCESTOR: a duplicated ancestor gives equal entries.  BY_PROBAND: a duplicated ancestor ID -> GENPHI_ERR_ARG
 *     (every path then has one end point: over all columns fewer than 2^48 paths, and sum S < 47 * 2^48 fits Int64);
 *   - an unknown ID in pro_ids or anc_ids -> GENPHI_ERR_UNKNOWN_ID (KeyError); n_pro = 0 or n_anc = 0: nothing is computed (the
 *     entries of a reduction over an empty list are 0, NaN, -1, -1).
 * Bounds.  The paths between one pair, as strings of father / mother choices, are prefix-free, so P <= 2^L for a longest ascent L
 * (Kraft), and L <= the level steps of the sweep.  The packed element holds P in 48 bits: create returns GENPHI_ERR_ARG for a sweep
 * of more than GENPHI_DEPTH_MAX_STEPS = 47 steps.  Then S <= 47 * 2^47 < 2^53 and the mean of a pair is the correctly rounded
 * quotient of exact operands.  BY_ANCESTOR: create returns GENPHI_ERR_ARG unless n_pro * max(steps, 1) * 2^steps < 2^63.
 *   create            host only (no GPU): checks IDs, pedigree order, depth and the bounds above, plans cuts, rows and slots.
 *                     panel_cols / panels_per_launch: the ancestor columns of a panel / the panels a launch covers; 0 = the default
 *                     rule (gc's rule on 16-byte elements: one panel's slot rows within about 150 MiB, at least 64 columns and a
 *                     multiple of 8; one panel per launch), any positive value is honoured (tests, A/B); negative -> GENPHI_ERR_ARG
 *   compute           the sweep on `device` (-1 = current); the result stays resident; GENPHI_ERR_ALLOC before any launch when the
 *                     result or the slot rows do not fit
 *   shape             rows x cols of the result: (n_pro, n_anc), (n_pro, 1) or (1, n_anc)
 *   result_device     device pointers of the four arrays and their common row pitch in entries (BY_PAIR: n_anc rounded up to a
 *                     multiple of 8, the entries [n_anc, ld) of a row are undefined; else cols)
 *   result_to_host    rows x cols entries each, row-major, packed; any of the four pointers may be NULL
 *   stats             device time of the last sweep (HIP events), its algorithmic bytes (source rows read and rows written at 16
 *                     bytes per panel column, plus 20 bytes per result entry and 24 per accumulator), the slot rows of one panel,
 *                     the panel width and the kernel launches of the sweep                                                     */
#define GENPHI_DEPTH_MAX_STEPS 47
#define GENPHI_DEPTH_BY_PAIR 0
#define GENPHI_DEPTH_BY_PROBAND 1
#define GENPHI_DEPTH_BY_ANCESTOR 2
typedef struct genphi_depth genphi_depth;
int genphi_depth_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                        int64_t n_pro, const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, int32_t by,
                        int32_t panel_cols, int32_t panels_per_launch, genphi_depth **out);
int genphi_depth_compute(genphi_depth *h, int32_t device);
int genphi_depth_shape(const genphi_depth *h, int64_t *rows, int64_t *cols);
int genphi_depth_result_device(const genphi_depth *h, const int16_t **d_min, const int16_t **d_max, const int64_t **d_paths,
                               const double **d_mean, int64_t *ld);
int genphi_depth_result_to_host(genphi_depth *h, int16_t *min, int16_t *max, int64_t *paths, double *mean);
int genphi_depth_stats(const genphi_depth *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *panel_cols,
                       int64_t *launches);
void genphi_depth_destroy(genphi_depth *h);

/* ---- gen.completeness and gen.depth: ascents by generation (csrc/completeness.hip, csrc/loader.cpp) ---------------------------
 * Replace completeness(pedigree, pro = pro(pedigree); genNo, type), src/describe.jl:73-125, and depth(pedigree), src/describe.jl:43-66.
 *
 * comp.  Entry [i][g] = the number of ascending paths of exactly g meioses that start at pro_ids[i] (the reference's
 * completeness[g] of that proband; 1 for g = 0), by the recursion P[x][0] = 1, P[x][g] = P[father][g - 1] + P[mother][g - 1] over
 * the generation cuts, on the host schedule of gen.gc / gen.occ (csrc/ancestor_sweep.h, every member of every cut has a row).
 * G = 1 + the longest ascent of any listed proband is the number of columns (1 when every proband is a founder).  Rules:
 *   - every proband gets its row, with or without children; a proband listed again gets the same row again;
 *   - an unknown ID in pro_ids -> GENPHI_ERR_UNKNOWN_ID (KeyError); n_pro = 0: G = 0 and an empty result.
 * Exactness.  Counts are Int64 and P[x][g] <= 2^g: create returns GENPHI_ERR_ARG for more than GENPHI_COMP_MAX_GENERATIONS = 62
 * generations above the probands (G > 63; the reference's own 2^row is an Int that turns negative at row 63).  The result is
 * Float64, converted on the device by the reference's two operations in its order, (double)count / 2^g * 100.0: bit-identical to
 * the reference's "IND" matrix at any permitted depth; generations beyond a proband's own depth are 0.0, generation 0 is 100.0.
 * Totals (what the reference's "MEAN" sums): per generation, the counts summed over the rows (each listed occurrence counts),
 * reduced on the device with 64-bit integer atomics (the same bits on every run).  A handle created with
 * GENPHI_COMP_FLAG_TOTALS_ONLY reduces the last step directly and never allocates an n_pro x G buffer.  A total is at most
 * n_pro 2^(G - 1): while (G - 1) + ceil(log2(n_pro)) <= 62 it cannot overflow; otherwise create with the flag, and totals on
 * any handle, return GENPHI_ERR_ARG and the caller sums the result rows instead.
 * MEAN from the totals: mean[g] = (double)totals[g] / 2^g * 100.0 / n_pro.  Every entry of the reference's matrix is
 * 25 count / 2^(g - 2), exact in Float64 while 25 count < 2^53, and so is every partial sum of a row of generation g while
 * 25 totals[g] < 2^53: the reference's sequential sum(matrix, dims = 2) is then exact in any order and the only rounding is the
 * final division.  So the mean is bit-identical to the reference whenever 25 totals[g] < 2^53 for every g; beyond that it is
 * within 2 ulp of the exact rational mean (three roundings of half an ulp: conversion, x 100, / n_pro), where the reference's own
 * sequential sum can be off by up to n_pro / 2 ulp.
 *   create            host only (no GPU): checks IDs, pedigree order and depth, plans cuts, rows and slots
 *   generations       G; valid after create
 *   compute           the sweep on `device` (-1 = current); the result stays resident; GENPHI_ERR_ALLOC before any launch when
 *                     the slot rows and the result do not fit
 *   result_device     device pointer and row pitch (ld = G) of the resident Float64 result (GENPHI_ERR_ARG on a totals-only handle)
 *   result_to_host    out: n_pro x G Float64, row-major: the finished percentages
 *   counts_to_host    out: n_pro x G Int64, row-major: the path counts
 *   totals            out: G Int64
 *   stats             device time of the last sweep (HIP events); its algorithmic bytes: 8 G (source rows read + slot rows
 *                     written) plus what the last list writes (16 n_pro G: counts and percentages; totals only: 8 G); the
 *                     slot rows; the entries of a slot row (G rounded up to 8); the kernel launches of the sweep
 *
 * genphi_genealogy_depth   gen.depth: 1 + the longest ascent of any individual (leaves_only = 0; founders count 1, an empty
 *                     pedigree 0), or of any individual without children (leaves_only = 1: what the reference's show prints).
 *                     One linear pass on the host where the reference recurses without memory; no order of the pedigree is
 *                     assumed.  Unknown parent -> GENPHI_ERR_UNKNOWN_ID, a cycle -> GENPHI_ERR_ARG.                          */
#define GENPHI_COMP_MAX_GENERATIONS 62
#define GENPHI_COMP_FLAG_TOTALS_ONLY 1   /* totals only: no n_pro x G result exists */
typedef struct genphi_comp genphi_comp;
int genphi_comp_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                       int64_t n_pro, const int64_t *pro_ids, int32_t flags, genphi_comp **out);
int genphi_comp_compute(genphi_comp *h, int32_t device);
int genphi_comp_generations(const genphi_comp *h, int32_t *generations);
int genphi_comp_result_device(const genphi_comp *h, const double **d_ptr, int64_t *ld);
int genphi_comp_result_to_host(genphi_comp *h, double *out);
int genphi_comp_counts_to_host(genphi_comp *h, int64_t *out);
int genphi_comp_totals(genphi_comp *h, int64_t *out);
int genphi_comp_stats(const genphi_comp *h, double *sweep_ms, double *algorithmic_bytes, int64_t *peak_slots, int32_t *row_entries,
                      int64_t *launches);
void genphi_comp_destroy(genphi_comp *h);
int genphi_genealogy_depth(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t *depth,
                           int32_t leaves_only);

/* ---- gen.implex: distinct ancestors by generation (csrc/implex.hip, csrc/implex.cpp) ---------------------------------------------
 * GENLIB's gen.implex; the reference has no form of it, so this text is the definition.  A_0(p) = {p}, A_{g+1}(p) = the known
 * parents of the members of A_g(p) (an individual can be in several A_g(p): generations overlap).
 *   counts[i][g] = |A_g(pro_ids[i])|, the DISTINCT ancestors at exactly g meioses, where gen.completeness counts them with
 *                  multiplicity (counts <= the counts of genphi_comp_*, equal while no ancestor repeats);
 *   GENPHI_IMPLEX_FLAG_ONLY_NEW: counts[i][g] = |A_g \ (A_0 u .. u A_{g-1})|, the individuals whose SHORTEST ascent from the
 *                  proband has g meioses (a breadth-first search); their sum over g >= 1 is the number of distinct ancestors.
 * G = 1 + the longest ascent of any listed proband, the same G as genphi_comp_generations for the same arguments.  Rules as for
 * comp: every proband gets its row, with or without children, each time it is listed; an unknown ID -> GENPHI_ERR_UNKNOWN_ID;
 * n_pro = 0: G = 0 and an empty result; more than GENPHI_IMPLEX_MAX_GENERATIONS generations above the probands -> GENPHI_ERR_ARG.
 * Method: rows are individuals, columns the listed probands as bits (64 per word).  The host plan lists per generation the union
 * frontier U_g (the individuals at exactly g meioses from ANY listed proband) and per row of U_g its children in U_{g-1}; a step
 * ORs the children's rows of the previous buffer into the row, a count kernel adds up the set bits per column.  Probands are
 * swept in panels of a multiple of 64 columns.  Everything is integer: the same bits on every run.  The percentages are
 * (double)count / 2^g * 100.0 in that order (generation 0 is 100.0, generations beyond a proband's depth 0.0).  A total is at most
 * n_pro n_ind < 2^62.  MEAN from the totals: (double)totals[g] / 2^g * 100.0 / n_pro; 25 totals[g] < 2^53 always holds here, so
 * everything before the division is exact and the mean is the correctly rounded exact rational.
 *   create            host only (no GPU): checks IDs, pedigree order and depth; builds U_g and the child lists, O(sum |U_g|)
 *   generations       G; valid after create
 *   frontier_rows     out: G Int64, |U_g|; host only, valid after create
 *   compute           the sweep on `device` (-1 = current); counts and percentages stay resident; GENPHI_ERR_ALLOC before any
 *                     launch when the frontier rows of even a 64-column panel and the result do not fit
 *   counts            out: n_pro x G Int64, row-major
 *   result_to_host    out: n_pro x G Float64, row-major: the finished percentages
 *   totals            out: G Int64: the column sums of the counts, reduced on the device (each listed occurrence counts)
 *   stats             device time of the last sweep (HIP events); its algorithmic bytes, sum over g of (|U_g| + child list
 *                     entries of U_g) x words of a panel row x 8, over the panels; G; the columns of a panel; the panels; the
 *                     lanes per row of the step kernel; the largest |U_g|                                                       */
#define GENPHI_IMPLEX_MAX_GENERATIONS 62
#define GENPHI_IMPLEX_FLAG_ONLY_NEW 1   /* onlyNewAnc: count an individual in the generation of its shortest ascent only */
typedef struct genphi_implex genphi_implex;
int genphi_implex_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                         int64_t n_pro, const int64_t *pro_ids, int32_t flags, genphi_implex **out);
int genphi_implex_compute(genphi_implex *h, int32_t device);
int genphi_implex_generations(const genphi_implex *h, int32_t *generations);
int genphi_implex_frontier_rows(const genphi_implex *h, int64_t *out);
int genphi_implex_counts(genphi_implex *h, int64_t *out);
int genphi_implex_result_to_host(genphi_implex *h, double *out);
int genphi_implex_totals(genphi_implex *h, int64_t *out);
int genphi_implex_stats(const genphi_implex *h, double *sweep_ms, double *algorithmic_bytes, int32_t *generations, int32_t *panel_cols,
                        int64_t *panels, int32_t *lanes_per_row, int64_t *peak_rows);
void genphi_implex_destroy(genphi_implex *h);

/* ---- gen.simuSample and gen.simuProb: gene dropping (csrc/simu.hip, csrc/simu.cpp, csrc/loader.cpp) ------------------------------
 * GENLIB's gen.simuSample and gen.simuProb; the reference has no form of them, so this text is the definition.  Marked alleles of
 * chosen ancestors are dropped down the pedigree S times and counted in the probands.
 * Inputs: a pedigree; pro_ids, the listed probands (any individuals, repeats allowed); anc_ids with anc_states, each 0, 1 or 2:
 * the copies of the marked allele the ancestor carries; simul_no = S >= 1; a 64-bit seed.
 * State.  Every individual x has two bit rows over the simulations, P_x and M_x: bit s of P_x says that in simulation s the copy
 * x received from its father is marked, M_x the same for its mother.  Simulation s is bit s % 64 of word w = s / 64.
 * Rules.
 *   - A listed ancestor with state t is fixed: t = 0: P = M = 0; t = 1: P = all ones, M = 0; t = 2: both all ones.  Its own
 *     parents are ignored: a listed ancestor blocks every path through it, a state-0 ancestor included.
 *   - Any other x with a known father f: P_x[w] = (T & P_f[w]) | (~T & M_f[w]) with T = R(seed, ID(x), 0, w); with a known
 *     mother m the same from P_m, M_m with T = R(seed, ID(x), 1, w).  An unknown parent gives a zero row.  Under selfing
 *     (father = mother) the two sides still draw independent words.
 *   - The count of x in simulation s is bit(P_x) + bit(M_x), in {0, 1, 2}.  Bits at positions >= S are never counted.
 * The random words.  R(seed, ID, side, w) is Philox4x32-10: multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, Weyl constants
 * 0x9E3779B9, 0xBB67AE85; a round is c <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)) and the key is bumped
 * after each round; key = (seed low 32, seed high 32), counter = (ID low 32, ID high 32, w >> 1, side).  Of the four 32-bit
 * outputs o0..o3, word w is o0 | o1 << 32 for even w and o2 | o3 << 32 for odd w: one block yields one 16-byte pair of words.
 * Known answers (counter; key; output): 0,0,0,0; 0,0; 6627e8d5 e169c58d bc57ac4c 9b00dbd8.  All ffffffff; all ffffffff;
 * 408f276d 41c83b0e a20bc7c6 6d5451fd.  243f6a88 85a308d3 13198a2e 03707344; a4093822 299f31d0; d16cfe09 94fdcceb 5001e420 24126ea1.
 * Invariants.  The stream is keyed on the individual's ID and the absolute word index, not on a rank, a position in a pruned
 * set, a panel or a launch: the result is a pure function of (pedigree relations, ancestors and states, seed).  So it does not
 * depend on how the simulations are split into panels; S = 64 gives the first 64 columns of S = 5000; a sub-list of probands
 * gives the same rows; pruning the pedigree to the paths between probands and ancestors first changes no row of the probands that pruning
 * keeps (it drops a proband below no listed ancestor, whose row is zero, and an ancestor above no listed proband, which marks no
 * row; a dropped ID is then unknown to the pruned pedigree).
 * Errors.  An unknown ID -> GENPHI_ERR_UNKNOWN_ID.  GENPHI_ERR_ARG: a state outside 0..2; an ancestor listed twice with
 * different states (equal repeats are allowed); S < 1 or S > GENPHI_SIMU_MAX_SIMULATIONS = 2^24; no probands; no ancestors.
 * Method.  The live set L = the individuals that are reachable downwards from a listed ancestor of state >= 1 without passing
 * through another listed ancestor (the carrier included) and that are a listed proband or an ancestor of one; everyone else has
 * zero rows for certain and gets no row.  level = 0 for the listed ancestors in L, else 1 + the largest level of the live
 * parents; one launch per level and panel.  Simulations are swept in panels of a multiple of 128 columns: one panel when the
 * rows (2 x n_live x pairs x 16 bytes) and the results fit the free device memory, else the widest that fits.
 *   create            host only (no GPU): checks IDs, states and pedigree order; plans L, the levels and the parent rows, O(n_ind).
 *                     GENPHI_SIMU_FLAG_NO_SAMPLE: no Int8 sample is allocated or written
 *   levels            n_live, the number of levels, and the rows of every level (room for that many); host only, any may be NULL
 *   rows              host only, any may be NULL: per row (n_live, ordered by level) the ID and the rows of its father and mother
 *                     (-1 = a zero row); per listed proband its row, -1 = not live (a row of zeros), or -2 - state for a listed
 *                     ancestor (its count is its state in every simulation)
 *   compute           the sweep on `device` (-1 = current); state counts and sample stay resident; GENPHI_ERR_ALLOC before any
 *                     launch when the rows of even a 128-column panel and the results do not fit
 *   sample_to_host    out: n_pro x S Int8, row-major: the count of proband i in simulation s; GENPHI_ERR_ARG under NO_SAMPLE
 *   state_counts      out: n_pro x 3 Int64, row-major: the simulations in which proband i carries 0, 1, 2 copies
 *   match_counts      state_pro: n_pro states in 0..2; out: S Int32: per simulation, the listed probands i whose count equals
 *                     state_pro[i].  May be called repeatedly with other states: a sweep of one panel left its rows resident
 *                     and they are only read; a sweep of several panels is swept again (the same bits) on every call
 *   stats             device time of the last compute (HIP events); its algorithmic bytes (per live row above level 0: two
 *                     parent rows read and one written, 32 bytes per pair of words, over the panels); the levels; the columns
 *                     of a panel; the panels; the lanes per row of the step kernel; n_live                                      */
#define GENPHI_SIMU_MAX_SIMULATIONS (1 << 24)
#define GENPHI_SIMU_FLAG_NO_SAMPLE 1   /* state and match counts only */
typedef struct genphi_simu genphi_simu;
int genphi_simu_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                       int64_t n_pro, const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, const int32_t *anc_states,
                       int64_t simul_no, uint64_t seed, int32_t flags, genphi_simu **out);
int genphi_simu_levels(const genphi_simu *h, int64_t *n_live, int32_t *levels, int64_t *rows_per_level);
int genphi_simu_rows(const genphi_simu *h, int64_t *row_ids, int32_t *father_rows, int32_t *mother_rows, int64_t *pro_positions);
int genphi_simu_compute(genphi_simu *h, int32_t device);
int genphi_simu_sample_to_host(genphi_simu *h, int8_t *out);
int genphi_simu_state_counts(genphi_simu *h, int64_t *out);
int genphi_simu_match_counts(genphi_simu *h, const int32_t *state_pro, int32_t *out);
int genphi_simu_stats(const genphi_simu *h, double *sweep_ms, double *algorithmic_bytes, int32_t *levels, int32_t *panel_cols,
                      int64_t *panels, int32_t *lanes_per_row, int64_t *n_live);
void genphi_simu_destroy(genphi_simu *h);

/* ---- gen.simuIdentity: identity coefficients by gene dropping (csrc/ident.hip, csrc/ident.cpp, csrc/label_sweep.h) ---------------
 * Jacquard's nine condensed identity states of every pair of probands, counted over S simulations in which every founder allele
 * is dropped down the pedigree under its own label.  The reference has no form of it, so this text is the definition.
 * Inputs.  A pedigree.  pro_ids, the listed probands: any individuals, at least one; repeats are allowed and give repeated rows
 * and columns.  simul_no = S with 1 <= S <= 2^24.  A 64-bit seed.
 * Live set.  The listed probands and all their ancestors.  level(x) = 0 when neither parent is known, else 1 + the largest level
 * of the known parents.  Rows are ordered by level, and by rank order within a level.
 * Founder alleles.  Every live x has two sides: 0 = the copy from the father, 1 = the copy from the mother.  A side whose parent
 * is unknown carries a founder allele; half-founders have one.  The allele table lists these (ID, side) pairs ascending by ID,
 * then side.  The label of an allele is its position in the table, n_labels is the table's length, and B = max(1, bit length of
 * n_labels - 1) planes.  (A live set has an individual without parents, so n_labels >= 2.)
 * State.  Per live x and simulation s there are two labels, LP_x[s] and LM_x[s].  Simulation s is bit s % 64 of word w = s / 64.
 * Rule.
 *   - A side with an unknown parent holds its own label in every simulation.
 *   - With a known father f: LP_x[s] = bit s of T ? LP_f[s] : LM_f[s], where T = R(seed, ID(x), 0, w).  With a known mother m
 *     the same from LP_m, LM_m with T = R(seed, ID(x), 1, w).
 *   - R is the gene-dropping word of this header (above), unchanged: the same Philox4x32-10, key, counter and word selection.
 *   - Under selfing the two sides draw independent words.  Nothing blocks a path: there are no listed ancestors.
 * Identity state.  For the ordered pair (i, j) of listed probands in simulation s, take a = LP_i, b = LM_i, c = LP_j, d = LM_j.
 * Jacquard's condensed states are
 *   1. a=b, c=d, a=c            4. a=b, c!=d, a not in {c, d}      7. a!=b, c!=d, {a, b} = {c, d}
 *   2. a=b, c=d, a!=c           5. a!=b, c=d, c in {a, b}          8. a!=b, c!=d, exactly one allele shared
 *   3. a=b, c!=d, a in {c, d}   6. a!=b, c=d, c not in {a, b}      9. a!=b, c!=d, none shared
 * The result is counts[i, j, k-1], the number of simulations s < S in state k: an Int32 array of n_pro x n_pro x 9, row-major.
 * Bits at positions >= S are never counted.
 * Invariants, all exact.  The nine counts of a pair add up to S.  counts[j, i] is counts[i, j] with the states 3 <-> 5 and
 * 4 <-> 6 exchanged.  A diagonal pair, or a pair of repeats of one ID, is in state 1 or 7 only.  The result is a pure function of
 * (pedigree relations, proband IDs, seed, S): it does not depend on the panel width; a sub-list of probands gives the sub-block;
 * gen.branching(ped, pro=P) first changes nothing; the label rows of S = 64 are the first 64 columns of those of S = 5000.
 * Cross-check with genphi_simu_*: list some individuals with both parents unknown as its ancestors with states 2 (or 1), under
 * the same seed; proband i's count in simulation s is then the number of its two labels that belong to those founders (state 1:
 * to their side-0 alleles).
 * Errors.  An unknown ID -> GENPHI_ERR_UNKNOWN_ID.  GENPHI_ERR_ARG: S out of range; no probands; n_pro^2 >= 2^31; n_labels >
 * 2^31 - 1; a negative panel_cols; an unknown flag.  GENPHI_ERR_ALLOC before any launch, when the device memory does not hold all
 * of the counts (36 n_pro^2 bytes), the optional labels and the rows of even a 128-column panel.
 * Method.  Plane b of a side is the bit row of bit b of its labels: a meiosis is (T & P_parent[b]) | (~T & M_parent[b]) on all B
 * planes with one T, one launch per level >= 1 and panel; two labels are equal where ~OR_b (x_b ^ y_b) is set.  The pair kernel
 * owns tiles of probands x probands and counts the states by popcounts of AND/OR combinations of the six equality words.
 *   create            host only (no GPU): checks IDs and pedigree order; plans the live set, the levels, the parent rows and the
 *                     allele table.  panel_cols: the simulations of a panel, 0 = the default (all of S, or the widest that fits
 *                     the device), else rounded up to a multiple of 128 and cut to S (tests, A/B).  flags: GENPHI_IDENT_FLAG_LABELS
 *                     keeps the probands' labels; GENPHI_IDENT_FLAG_ALL_PAIRS computes every ordered pair instead of the pairs
 *                     of tiles on or above the diagonal plus their mirror images (the same result; the A/B of the bench)
 *   levels            n_live, the number of levels, and the rows of every level (room for that many); host only, any may be NULL
 *   alleles           n_labels, B, and the table as IDs and sides (room for n_labels each); host only, any may be NULL
 *   compute           the sweep on `device` (-1 = current); counts (and labels) stay resident
 *   counts_to_host    out: n_pro x n_pro x 9 Int32, row-major
 *   labels_to_host    out: n_pro x 2 x S Int32, row-major: LP and LM of proband i; GENPHI_ERR_ARG without GENPHI_IDENT_FLAG_LABELS
 *   stats             of the last compute, by HIP events: the device time of init and level steps, and of gather and pair kernel,
 *                     summed over the panels; the algorithmic bytes of the steps (per side with a known parent: two runs of B
 *                     planes read and one written, 16 bytes per plane and pair of words); the word operations of the pair kernel
 *                     (ordered pairs computed -- n_pro (n_pro + 1) / 2, or n_pro^2 under ALL_PAIRS -- x words x (12 B + 40));
 *                     levels; the columns of a panel; the panels; B; the pair kernel's tile rows and columns; the lanes per row
 *                     of the step kernel                                                                                      */
#define GENPHI_IDENT_FLAG_LABELS 1
#define GENPHI_IDENT_FLAG_ALL_PAIRS 2
typedef struct genphi_ident genphi_ident;
int genphi_ident_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                        int64_t n_pro, const int64_t *pro_ids, int64_t simul_no, uint64_t seed, int32_t panel_cols, int32_t flags,
                        genphi_ident **out);
int genphi_ident_levels(const genphi_ident *h, int64_t *n_live, int32_t *levels, int64_t *rows_per_level);
int genphi_ident_alleles(const genphi_ident *h, int64_t *n_labels, int32_t *planes, int64_t *ids, int32_t *sides);
int genphi_ident_compute(genphi_ident *h, int32_t device);
int genphi_ident_counts_to_host(genphi_ident *h, int32_t *out);
int genphi_ident_labels_to_host(genphi_ident *h, int32_t *out);
int genphi_ident_stats(const genphi_ident *h, double *sweep_ms, double *pair_ms, double *algorithmic_bytes, double *word_ops,
                       int32_t *levels, int32_t *panel_cols, int64_t *panels, int32_t *planes, int32_t *tile_rows, int32_t *tile_cols,
                       int32_t *lanes_per_row);
void genphi_ident_destroy(genphi_ident *h);

/* ---- gen.simuRetention: founder allele survival by gene dropping (csrc/retain.hip, csrc/retain.h, csrc/label_sweep.h) --------------
 * The question gene dropping was made for (MacCluer et al. 1986): which founder alleles are still present in the listed probands,
 * and how many.  Retention has no closed form on a general pedigree and does not follow from the kinship matrix or from the pair
 * counts of gen.simuIdentity.  The reference has no form of it, so this text is the definition, and it is this package's own.
 * Inputs, live set, levels, rows, allele table, labels LP_x[s] / LM_x[s], the rule and the random word R are those of
 * genphi_ident_* above, word for word: under the same pedigree, probands, seed and S the labels are the same labels.  Repeats in
 * the proband list are allowed.
 * present(l, s) holds when some listed proband carries label l on either side in simulation s.  The results:
 *   survived[l]   Int32 x n_labels: the number of s < S with present(l, s).
 *   both[l]       Int32 x n_labels.  It applies where labels l and l + 1 belong to the same ID, that is, a founder with both
 *                 parents unknown, l being its side 0: the number of s < S with present(l, s) and present(l + 1, s), stored at
 *                 l.  Every other entry is 0.
 *   distinct[s]   Int32 x S: the number of labels l with present(l, s).
 * Bits at positions >= S are never counted.
 * Invariants, all exact.
 *   1. The sum of distinct over s equals the sum of survived over l.
 *   2. 1 <= distinct[s] <= min(n_labels, 2 x the number of different listed IDs).
 *   3. both[l] <= min(survived[l], survived[l + 1]), and survived[l] + survived[l + 1] - both[l] <= S.
 *   4. The label of a founder side whose carrier is itself listed has survived = S.
 *   5. The result is a pure function of the pedigree relations, the SET of listed IDs (order and repeats of the list change
 *      nothing), the seed and S.
 *   6. The result does not depend on the panel width or on the label chunk.
 *   7. distinct at S = 64 is the first 64 entries of distinct at S = 5000.
 *   8. gen.branching(ped, pro=P) first changes nothing.
 *   9. Matched through (ID, side), survived of a proband set is entrywise <= survived of a superset under the same seed.
 *  10. The three arrays equal the same reductions of genphi_ident_labels_to_host for the same arguments.
 * Errors.  Those of genphi_ident_create without the n_pro^2 >= 2^31 refusal (a list that gen.simuIdentity refuses is planned
 * here), plus a negative chunk_labels and both form flags at once -> GENPHI_ERR_ARG.  GENPHI_ERR_ALLOC from compute before any
 * launch, when the device does not hold the results (8 n_labels + 4 S bytes), the lists and the rows of even a 128-column panel.
 * Only 2 n_labels + S integers ever move to the host.
 * Method.  The label sweep of genphi_ident_* (its init and step kernels, shared), then one mark kernel per panel that reads the
 * listed probands' rows in place.  A workgroup owns the 64 simulations of a word and a chunk of the labels; it keeps one bitmap per
 * simulation in LDS, decodes every proband side once, sets bits, and reduces the bitmaps by popcounts and wave ballots into
 * integer adds (csrc/retain.hip).
 *   create            host only (no GPU): ident's checks and plan.  panel_cols as for genphi_ident_create.  chunk_labels: the labels
 *                     of a chunk, 0 = the default (the whole table up to 8,192 labels, else 8,192), else rounded up to a multiple
 *                     of 32 and cut to n_labels and to 16,384 (tests, A/B).  flags: GENPHI_RETAIN_FLAG_PLAIN_OR marks with an
 *                     unconditional LDS atomic OR, GENPHI_RETAIN_FLAG_TEST_FIRST reads the word first and skips the atomic when the
 *                     bit is set already; neither = the form that ships (the same result; the A/B of the bench)
 *   levels, alleles   as genphi_ident_levels and genphi_ident_alleles
 *   compute           the sweep on `device` (-1 = current); the three arrays stay resident
 *   survived_to_host, both_to_host    out: n_labels Int32
 *   distinct_to_host  out: S Int32
 *   stats             of the last compute, by HIP events: the device time of init and level steps, and of the mark kernel, summed
 *                     over the panels; the algorithmic bytes of the steps (as genphi_ident_stats); the bytes of the probands' planes
 *                     the mark kernel reads (2 n_pro x B x 16 per pair of words and chunk); levels; the columns of a panel; the
 *                     panels; B; the labels of a chunk; the chunks; the LDS bytes of a workgroup of the mark kernel; the lanes per
 *                     row of the step kernel                                                                                   */
#define GENPHI_RETAIN_FLAG_PLAIN_OR 1
#define GENPHI_RETAIN_FLAG_TEST_FIRST 2
typedef struct genphi_retain genphi_retain;
int genphi_retain_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                         int64_t n_pro, const int64_t *pro_ids, int64_t simul_no, uint64_t seed, int32_t panel_cols,
                         int32_t chunk_labels, int32_t flags, genphi_retain **out);
int genphi_retain_levels(const genphi_retain *h, int64_t *n_live, int32_t *levels, int64_t *rows_per_level);
int genphi_retain_alleles(const genphi_retain *h, int64_t *n_labels, int32_t *planes, int64_t *ids, int32_t *sides);
int genphi_retain_compute(genphi_retain *h, int32_t device);
int genphi_retain_survived_to_host(genphi_retain *h, int32_t *out);
int genphi_retain_both_to_host(genphi_retain *h, int32_t *out);
int genphi_retain_distinct_to_host(genphi_retain *h, int32_t *out);
int genphi_retain_stats(const genphi_retain *h, double *sweep_ms, double *mark_ms, double *algorithmic_bytes, double *mark_bytes,
                        int32_t *levels, int32_t *panel_cols, int64_t *panels, int32_t *planes, int32_t *chunk_labels,
                        int64_t *chunks, int32_t *lds_bytes, int32_t *lanes_per_row);
void genphi_retain_destroy(genphi_retain *h);

/* ---- gen.simuCarriers: the carriers of every founder allele among listed cases (csrc/carry.hip, csrc/carry.h, csrc/label_sweep.h) --
 * A set of affected probands carries a rare variant: which founder allele most probably introduced it, and how many of the listed
 * probands does one founder allele reach?  GENLIB's gen.simuProb answers for one ancestor per call; here every founder allele is
 * answered by one sweep.  The reference has no form of it, so this text is the definition, and it is this package's own.
 * Inputs.  A pedigree; the cases, at least one individual; the controls, an optional second list of individuals that must not carry
 * the allele; S and a 64-bit seed.  Both lists count as SETS: order and repeats change nothing.  An individual in both lists is
 * GENPHI_ERR_ARG.  The listed probands of the plan are the cases followed by the controls: live set, levels, rows, allele table,
 * labels LP_x[s] / LM_x[s], the rule and the random word R are those of genphi_ident_* above, word for word.  The same (pedigree
 * relations, seed) therefore gives the same realisation as gen.simuIdentity, gen.simuRetention and gen.simuSharing.
 * Let n be the number of distinct cases.  Per simulation s < S and label l:
 *   c1(l, s) = the distinct cases with at least one side equal to l,
 *   c2(l, s) = the distinct cases with both sides equal to l,
 *   x(l, s)  = 1 when some control has a side equal to l, else 0.
 * With W = min(n, max_count) + 1 columns (max_count = 0: W = n + 1; the last column lumps only when max_count < n) the results:
 *   excluded[l]                       Int32 x n_labels: the s with x = 1.
 *   carriers[l, min(c1, W - 1)]       Int32 x n_labels x W, row-major: the s with x = 0 and c1 >= 1.
 *   homozygotes[l, min(c2, W - 1)]    Int32 x n_labels x W, row-major: the s with x = 0 and c2 >= 1.
 * The device never writes column 0 of either table: it stays 0 in what carriers_to_host and homozygotes_to_host deliver, and the
 * Python layer fills both as S - excluded[l] - (the sum of the columns c >= 1).  Bits at positions >= S are never counted.
 * Invariants, all exact.
 *   1. With no controls the sum over c >= 1 of carriers[l, c] equals survived[l] of genphi_retain_* for the same pedigree, cases,
 *      seed and S.
 *   2. With no controls and W = n + 1 the sum over l and c of c (carriers[l, c] + homozygotes[l, c]) is 2 n S: every side of every
 *      case carries one label.
 *   3. The sum over c of c homozygotes[l, c] <= the sum over c of c carriers[l, c] for every l, at any W.
 *   4. Both alleles of a case that is itself a founder have the sum over c >= 1 of carriers equal to S - excluded.
 *   5. The bytes do not depend on the panel width, the label chunk, or the order and repeats of either list.
 *   6. Keyed by (ID, side), excluded equals survived of genphi_retain_* run on the controls alone under the same seed (the two
 *      allele tables differ: on the common keys).
 *   7. Keyed by (ID, side), adding controls never raises a cell of carriers or homozygotes with c >= 1.
 * Errors.  Those of genphi_ident_create without the n_pro^2 >= 2^31 refusal.  GENPHI_ERR_ARG, all in create before any device work:
 * no cases; an individual in both lists; n > 32,767; n_labels x W > 2^31 - 1; S outside 1 .. 2^24; a negative panel_cols,
 * chunk_labels or max_count.  GENPHI_ERR_ALLOC from compute before any launch, when the device does not hold the results
 * (4 n_labels (2 W + 1) bytes), the lists and the rows of even a 128-column panel.
 * Method.  The label sweep of genphi_ident_* (its init and step kernels, shared), then one count kernel per panel that reads the
 * rows of the cases and the controls in place.  A workgroup owns the 64 simulations of a word and a chunk of the labels; it keeps
 * one counter dword per (simulation, label) in LDS (c1 in bits 0-15, c2 in bits 16-30, x in bit 31: n <= 32,767 keeps the fields
 * apart), decodes both sides of every listed individual once, adds by LDS atomics, and reduces the dwords into integer adds
 * (csrc/carry.hip).
 *   create            host only (no GPU): ident's checks and plan on the cases followed by the controls; the lists as sets; the
 *                     limits.  panel_cols as for genphi_ident_create.  chunk_labels: the labels of a chunk, 0 = the default (608,
 *                     the most that 160 KiB of LDS hold), else rounded up to a multiple of 32 and cut to 608; either is cut to n_labels
 *                     (tests, A/B).  max_count: 0 = a column for every count, else the last column W - 1 = min(n, max_count)
 *                     holds every count at or above it
 *   levels, alleles   as genphi_ident_levels and genphi_ident_alleles
 *   compute           the sweep on `device` (-1 = current); the three arrays stay resident
 *   carriers_to_host, homozygotes_to_host    out: n_labels x W Int32, row-major, column 0 zero
 *   excluded_to_host  out: n_labels Int32
 *   stats             of the last compute, by HIP events: the device time of init and level steps, and of the count kernel, summed
 *                     over the panels; the algorithmic bytes of the steps (as genphi_ident_stats); the bytes of the listed rows'
 *                     planes the count kernel reads (2 (n + controls) x B x 16 per pair of words and chunk); levels; the columns
 *                     of a panel; the panels; B; the labels of a chunk; the chunks; the LDS bytes of a workgroup of the count
 *                     kernel; W; n; the distinct controls                                                                      */
typedef struct genphi_carry genphi_carry;
int genphi_carry_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                        int64_t n_cases, const int64_t *case_ids, int64_t n_controls, const int64_t *control_ids, int64_t simul_no,
                        uint64_t seed, int32_t panel_cols, int32_t chunk_labels, int32_t max_count, genphi_carry **out);
int genphi_carry_levels(const genphi_carry *h, int64_t *n_live, int32_t *levels, int64_t *rows_per_level);
int genphi_carry_alleles(const genphi_carry *h, int64_t *n_labels, int32_t *planes, int64_t *ids, int32_t *sides);
int genphi_carry_compute(genphi_carry *h, int32_t device);
int genphi_carry_carriers_to_host(genphi_carry *h, int32_t *out);
int genphi_carry_homozygotes_to_host(genphi_carry *h, int32_t *out);
int genphi_carry_excluded_to_host(genphi_carry *h, int32_t *out);
int genphi_carry_stats(const genphi_carry *h, double *sweep_ms, double *count_ms, double *algorithmic_bytes, double *count_bytes,
                       int32_t *levels, int32_t *panel_cols, int64_t *panels, int32_t *planes, int32_t *chunk_labels,
                       int64_t *chunks, int32_t *lds_bytes, int32_t *columns, int32_t *n_cases, int32_t *n_controls);
void genphi_carry_destroy(genphi_carry *h);

/* ---- gen.simuOrigins: which founders the kinship and the inbreeding come from (csrc/origin.hip, csrc/origin.h, csrc/label_sweep.h) --
 * Which founder alleles do the identical-by-descent alleles of two probands descend from: within a group of probands, between two
 * groups, and in the inbreeding of the probands themselves?  This is Lacy's partition of kinship and inbreeding by founder; its
 * inbreeding half is the partial inbreeding coefficients of Lacy, Alaks & Walsh (1996).  The exact recursion is one kinship sweep per
 * founder; the field computes it by gene dropping.  The reference has no form of it, so this text is the definition, and it is this
 * package's own.
 * Inputs.  A pedigree; a list of probands, at least one, which counts as a SET; group[k], per listed entry an Int32 in -1 .. G - 1
 * (NULL: everyone is in group 0 and G = 1); G in 1 .. 32; S in 1 .. 2^24 and a 64-bit seed.  A proband with group -1 stays in the
 * plan, so the realisation does not change; it is counted nowhere.  An ID listed twice with two different groups (-1 counts as one)
 * is GENPHI_ERR_ARG.  On the list as given the live set, levels, rows, allele table, labels LP_x[s] / LM_x[s], the rule and the random
 * word R are those of genphi_ident_* above, word for word.  The same (pedigree relations, seed) therefore gives the same realisation
 * as gen.simuIdentity, gen.simuRetention, gen.simuCarriers and gen.simuSharing.
 * Let n_a be the number of distinct probands of group a, and n the number of distinct probands in any group, ordered by first
 * appearance in the list.  Per simulation s < S, label l and group a:
 *   c1_a(l, s) = the distinct probands of a with at least one side equal to l,
 *   c2_a(l, s) = those with both sides equal to l,
 *   k_a  = c1_a + c2_a, the gene copies of l in a,
 *   m_aa = (k_a^2 - c1_a - 3 c2_a) / 2, the matching copy pairs between two DIFFERENT probands of a (the sum over i < j of k_i k_j),
 *   m_ab = k_a k_b for a < b.
 * With P = G (G + 1) / 2 and p numbering the pairs a <= b row-major over the upper triangle (p = a G - a (a - 1) / 2 + b - a):
 *   copies[a, l]           Int64 x G x n_labels, row-major: the sum over s of k_a.
 *   autozygous[a, l]       Int64 x G x n_labels: the sum over s of c2_a.
 *   matches[p, l]          Int64 x P x n_labels: the sum over s of m_ab.
 *   autozygous_pro[i, l]   Int32 x n x n_labels, only when requested: the s in which both sides of distinct proband i equal l.
 * Bits at positions >= S are never counted.  Word sizes: k <= 65,534, so a term of one simulation is below 2^32; a sum over
 * simulations is not: every accumulation past a single term is 64-bit.
 * Invariants, all exact integers.
 *   1. The sum over l of copies[a, l] is 2 n_a S: every side of every proband carries one label.
 *   2. With G = 1 and the same list, seed and S, for genphi_carry_* with no controls and W = n + 1: copies[0, l] is the sum over c of
 *      c (carriers[l, c] + homozygotes[l, c]), and autozygous[0, l] is the sum over c of c homozygotes[l, c].
 *   3. Against genphi_ident_* on the distinct probands, same seed and S: the sum over l of matches[(a, b), l] equals
 *      4 n1 + 2 (n3 + n5 + n7) + n8 of its counts, summed over the pairs i < j within a, or over i in a and j in b (the numerator of
 *      the kinship of gen.simuIdentity); the sum over l of autozygous[a, l] equals the sum over i in a of counts[i, i, 0].
 *   4. Merging groups adds.  For a union A of groups, copies and autozygous of A are the sums over its parts, and matches[(A, A)] is
 *      the sum over a in A of m_aa plus the sum over a < b in A of m_ab: every grouping agrees with G = 1.
 *   5. The sum over i in a of autozygous_pro[i, l] is autozygous[a, l].
 *   6. A listed founder has autozygous_pro = 0 and, from itself, S copies at each of its own labels; two distinct founders alone in
 *      their groups have matches = 0 between them.
 *   7. The bytes do not depend on the panel width, the label chunk, the order or the repeats of the list, or on whether
 *      autozygous_pro is requested; renumbering the groups permutes the tables.
 * Errors.  Those of genphi_ident_create without the n_pro^2 >= 2^31 refusal.  GENPHI_ERR_ARG, all in create before any device work:
 * no probands, or none in a group; G outside 1 .. 32 (NULL group: G must be 1); a group outside -1 .. G - 1; an ID with two groups;
 * n_a > 32,767 for some a; n x n_labels > 2^31 - 1 when autozygous_pro is requested; S outside 1 .. 2^24; a negative panel_cols or
 * chunk_labels; by_proband other than 0 or 1.  GENPHI_ERR_ALLOC from compute before any launch, when the device does not hold the
 * tables (8 n_labels (2 G + P) bytes, and 4 n n_labels), the lists and the rows of even a 128-column panel.
 * Method.  The label sweep of genphi_ident_* (its init and step kernels, shared), then one count kernel per panel that reads the rows
 * of the grouped probands in place and never looks at a pair.  A workgroup owns the 64 simulations of a word and a chunk of the
 * labels; it keeps one counter dword per (simulation, label, group) in LDS (c1 in bits 0-15, c2 in bits 16-30: n_a <= 32,767 keeps
 * the fields apart), decodes both sides of every grouped proband once, adds by LDS atomics, and after a barrier forms k, c2, m_aa and
 * m_ab per simulation in 64 bits, sums them over the wave and adds them into the tables with 64-bit integer atomics
 * (csrc/origin.hip).  Not offered: origins per pair of probands, the exact partial kinship (one sweep per founder), linked loci,
 * more than one device.
 *   create            host only (no GPU): ident's checks and plan on the list as given; the list as a set with its groups; the
 *                     limits.  panel_cols as for genphi_ident_create.  chunk_labels: the labels of a chunk, 0 = the default (the
 *                     widest: the largest LC with 256 ((LC G) | 1) <= 163,840 bytes of LDS, 639 / G), else as given; either is cut
 *                     to the widest and to n_labels (tests, A/B).  by_proband: 1 = keep autozygous_pro
 *   levels, alleles   as genphi_ident_levels and genphi_ident_alleles
 *   compute           the sweep on `device` (-1 = current); the tables stay resident
 *   copies_to_host, autozygous_to_host    out: G x n_labels Int64, row-major
 *   matches_to_host   out: P x n_labels Int64, row-major
 *   by_proband_to_host    out: n x n_labels Int32, row-major; GENPHI_ERR_ARG unless created with by_proband
 *   stats             of the last compute, by HIP events: the device time of init and level steps, and of the count kernel, summed
 *                     over the panels; the algorithmic bytes of the steps (as genphi_ident_stats); the bytes of the grouped rows'
 *                     planes the count kernel reads (2 n x B x 16 per pair of words and chunk); levels; the columns of a panel; the
 *                     panels; B; the labels of a chunk; the chunks; the LDS bytes of a workgroup of the count kernel; G; n          */
typedef struct genphi_origin genphi_origin;
int genphi_origin_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                         int64_t n_pro, const int64_t *pro_ids, const int32_t *group, int32_t n_groups, int64_t simul_no,
                         uint64_t seed, int32_t panel_cols, int32_t chunk_labels, int32_t by_proband, genphi_origin **out);
int genphi_origin_levels(const genphi_origin *h, int64_t *n_live, int32_t *levels, int64_t *rows_per_level);
int genphi_origin_alleles(const genphi_origin *h, int64_t *n_labels, int32_t *planes, int64_t *ids, int32_t *sides);
int genphi_origin_compute(genphi_origin *h, int32_t device);
int genphi_origin_copies_to_host(genphi_origin *h, int64_t *out);
int genphi_origin_autozygous_to_host(genphi_origin *h, int64_t *out);
int genphi_origin_matches_to_host(genphi_origin *h, int64_t *out);
int genphi_origin_by_proband_to_host(genphi_origin *h, int32_t *out);
int genphi_origin_stats(const genphi_origin *h, double *sweep_ms, double *count_ms, double *algorithmic_bytes, double *count_bytes,
                        int32_t *levels, int32_t *panel_cols, int64_t *panels, int32_t *planes, int32_t *chunk_labels,
                        int64_t *chunks, int32_t *lds_bytes, int32_t *n_groups, int32_t *n_grouped);
void genphi_origin_destroy(genphi_origin *h);

/* ---- gen.simuUniqueness: the genome uniqueness of every proband (csrc/unique.hip, csrc/unique.h, csrc/label_sweep.h) ---------------
 * For each proband, how much of what it carries is carried by nobody else, and what is lost when it goes?  That is the genome
 * uniqueness of MacCluer et al. (1986), the statistic by which individuals are ranked for breeding, sampling or sequencing.  It has no
 * closed form on a general pedigree and follows neither from the kinship matrix nor from the tables of genphi_carry_* (which know that
 * an allele has one carrier, not who) or genphi_origin_* (which know who is autozygous, not who else carries the allele).  The
 * reference has no form of it, so this text is the definition, and it is this package's own.
 * Inputs.  A pedigree; pro, the evaluated probands, at least one; others, an optional second list of individuals that count as
 * carriers but are not evaluated (the rest of the living population); S and a 64-bit seed.  Both lists count as SETS: order and
 * repeats change nothing.  An individual in both lists is a proband, not an error.  The POPULATION is the distinct probands in
 * ascending row order, followed by the distinct others that are not probands; n is the number of distinct probands, n_pop the size of
 * the population.  The listed probands of the plan are pro followed by others: live set, levels, rows, allele table, labels
 * LP_x[s] / LM_x[s], the rule and the random word R are those of genphi_ident_* above, word for word.  The same (pedigree relations,
 * seed) therefore gives the same realisation as gen.simuIdentity, gen.simuRetention, gen.simuCarriers and gen.simuOrigins.
 * Per simulation s < S and label l:
 *   c1(l, s) = the distinct members of the population with at least one side equal to l (genphi_carry_*'s c1 with the population as
 *              the cases).
 * With K = min(n_pop, max_share) columns (max_share = 0: K = n_pop), column min(m, K) - 1 holds share m, so the last column lumps
 * every m >= K when K < n_pop.  With a and b the two sides of proband i in simulation s, the results:
 *   alleles[i, .]      Int32 x n x K, row-major.  a != b: one count at the column of c1(a, s) and one at the column of c1(b, s);
 *                      a = b: one count at the column of c1(a, s).
 *   autozygous[i, .]   Int32 x n x K, row-major.  a = b: one count at the column of c1(a, s).
 * Row i is the i-th distinct proband in ascending row order; genphi_unique_probands reports the IDs in that order.  Bits at
 * positions >= S are never counted.
 * Invariants, all exact.
 *   1. For every i the sum of alleles[i, :] plus the sum of autozygous[i, :] is 2 S: every side carries one label.
 *   2. With no others and K = n, for genphi_carry_* on the same probands as cases, no controls, the same seed and S, and W = n + 1:
 *      the sum over i of alleles[i, m - 1] is m times the sum over l of carriers[l, m], for every m; and the sum over i and m of
 *      autozygous[i, m] is the sum over l and c of c homozygotes[l, c].
 *   3. With no others and K = n: every sum over i of alleles[i, m - 1] is divisible by m, and the sum over m of the quotients is
 *      the sum over s of distinct[s] of genphi_retain_*: every surviving allele is shared out among its carriers exactly once.
 *   4. The sum over m of autozygous[i, m] is the sum over l of autozygous_pro[i, l] of genphi_origin_* with by_proband, and the
 *      inbreeding count counts[i, i, 0] of genphi_ident_* of that proband.
 *   5. The bytes do not depend on the panel width, the label chunk, or the order and repeats of either list.
 *   6. Keyed by proband ID, adding others never lowers a share: for every i and m the sum over m' <= m of alleles[i, m'] does not
 *      rise, and the same holds for autozygous.
 *   7. A proband that is a founder, has no descendant in the population and is listed alone with any others has alleles[i, 0] = 2 S
 *      when K > 1 (K = 1: everything is in the one column).  A proband whose two parents are both in the population has
 *      alleles[i, 0] = 0 when K > 1.
 *   8. A smaller max_share gives the same leading K - 1 columns; its last column is the sum of the dropped ones.
 * Errors.  Those of genphi_ident_create without the n_pro^2 >= 2^31 refusal.  GENPHI_ERR_ARG, all in create before any device work:
 * no probands; n_pop > 65,535 (the counters are 16 bits); n x K > 2^31 - 1 cells ("pass a smaller maxShare"); S outside 1 .. 2^24; a
 * negative panel_cols, chunk_labels or max_share.  GENPHI_ERR_ALLOC from compute before any launch, when the device does not hold
 * the results (8 n K bytes), the lists and the rows of even a 128-column panel.
 * Method.  The label sweep of genphi_ident_* (its init and step kernels, shared), then one count kernel per panel that reads the
 * rows of the population in place.  A workgroup owns the 64 simulations of a word and a chunk of the labels; it keeps one 16-bit
 * counter per (simulation, label) in LDS, two to a dword (n_pop <= 65,535 keeps the halves apart), decodes both sides of every
 * member of the population once and adds by LDS atomics; after a barrier it decodes the probands again, reads the counter of each
 * side whose label lies in the chunk and adds 1 at the cell of that share by integer atomics, the lanes of a wave that meet in one
 * of the first columns counted by a ballot first (csrc/unique.hip).  Not offered: uniqueness within groups; the simulations in which
 * a proband is the sole carrier of at least one allele (that does not add over label chunks); linked loci; more than one device.
 *   create            host only (no GPU): ident's checks and plan on pro followed by others; the lists as sets; the limits.
 *                     panel_cols as for genphi_ident_create.  chunk_labels: the labels of a chunk, 0 = the default, else rounded up
 *                     to a multiple of 64 and cut to 1,216 (the most that 160 KiB of LDS hold); either is cut to n_labels (tests,
 *                     A/B).  max_share: 0 = a column for every share, else the last column K - 1 = min(n_pop, max_share) - 1 holds
 *                     every share at or above max_share
 *   levels, alleles   as genphi_ident_levels and genphi_ident_alleles
 *   probands          n and, when ids is not NULL, the IDs of the rows of the two tables (n of them)
 *   compute           the sweep on `device` (-1 = current); the two tables stay resident
 *   alleles_to_host, autozygous_to_host    out: n x K Int32, row-major
 *   stats             of the last compute, by HIP events: the device time of init and level steps, and of the count kernel, summed
 *                     over the panels; the algorithmic bytes of the steps (as genphi_ident_stats); the bytes of the rows' planes the
 *                     count kernel reads (2 (n_pop + n) x B x 16 per pair of words and chunk); levels; the columns of a panel; the
 *                     panels; B; the labels of a chunk; the chunks; the LDS bytes of a workgroup of the count kernel; K; n; n_pop */
typedef struct genphi_unique genphi_unique;
int genphi_unique_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                         int64_t n_pro, const int64_t *pro_ids, int64_t n_others, const int64_t *other_ids, int64_t simul_no,
                         uint64_t seed, int32_t panel_cols, int32_t chunk_labels, int32_t max_share, genphi_unique **out);
int genphi_unique_levels(const genphi_unique *h, int64_t *n_live, int32_t *levels, int64_t *rows_per_level);
int genphi_unique_alleles(const genphi_unique *h, int64_t *n_labels, int32_t *planes, int64_t *ids, int32_t *sides);
int genphi_unique_probands(const genphi_unique *h, int64_t *n, int64_t *ids);
int genphi_unique_compute(genphi_unique *h, int32_t device);
int genphi_unique_alleles_to_host(genphi_unique *h, int32_t *out);
int genphi_unique_autozygous_to_host(genphi_unique *h, int32_t *out);
int genphi_unique_stats(const genphi_unique *h, double *sweep_ms, double *count_ms, double *algorithmic_bytes, double *count_bytes,
                        int32_t *levels, int32_t *panel_cols, int64_t *panels, int32_t *planes, int32_t *chunk_labels,
                        int64_t *chunks, int32_t *lds_bytes, int32_t *columns, int32_t *n, int32_t *n_pop);
void genphi_unique_destroy(genphi_unique *h);

/* ---- gen.simuSharing: linked-locus gene dropping and IBD segments (csrc/link.hip, csrc/link.cpp, csrc/label_sweep.h) ---------------
 * gen.simuIdentity above drops every founder allele at ONE locus.  Here a simulation is a chromosome of L linked loci: a meiosis
 * copies a mosaic of the parent's two chromosomes, and the sharing of a pair of probands is read off locus by locus: how much of the
 * chromosome they share identical by descent (IBD) in one realisation, how much that varies, and in how many segments it comes.
 * GENLIB's gen.simuHaplo is the model; the reference has no form of it, so this text is the definition, and it is this package's own.
 * Inputs.  A pedigree and pro_ids, the listed probands, with the rules of genphi_ident_create.  loci = L with 1 <= L <= 4096;
 * W = ceil(L / 64) words per chromosome.  q with 0 <= q <= 32768: the recombination probability between neighbouring loci is
 * r = q / 65536 exactly; q = 32768 gives independent loci, q = 0 no recombination.  simul_no = S with 1 <= S <= 2^24.  A 64-bit
 * seed.  panel_sims: 0 = the default rule, else the simulations of a panel.  Flags: LABELS and ALL_PAIRS, as for ident.
 * Live set, levels, rows, allele table, n_labels and B are those of genphi_ident_* for the same pedigree and probands.
 * Random words.  For individual ID, side (0 = the copy from the father), simulation s and chromosome word w < W, block d is
 * Philox4x32-10 with the counter (ID low, ID high, s, 0x80000000 | side | w << 1 | d << 8) and the key (seed low, seed high).  Bit 31
 * of the last counter word keeps these streams disjoint from the gene-dropping word (there the word is 0 or 1) and from the
 * bootstrap's (2).  U_2d = o0 | o1 << 32 and U_2d+1 = o2 | o3 << 32 of block d, for d = 0 .. 7.
 * Crossover word.  acc = 0; for t = 0 .. 15, with q_t = bit t of q: acc = q_t ? (acc | U_t) : (acc & U_t); X(w) = acc.  Every bit
 * of X(w) is set with probability q / 65536 exactly, independently of the others.  Blocks below the lowest set bit of q leave
 * acc at 0 and may be skipped.  In word 0, bit 0 of X is replaced by bit 0 of U_16 (block d = 8): the strand the copy starts on, a
 * fair coin.  Bit k of the chromosome is bit k % 64 of word k / 64.
 * Transmission word.  T is the inclusive prefix XOR of X along the whole chromosome: T[k] = X[0] ^ .. ^ X[k].
 * Rule.
 *   - A side with an unknown parent holds its own label at every locus of every simulation.
 *   - With a known father f: LP_x[s, k] = T[k] ? LP_f[s, k] : LM_f[s, k], with the T of (ID(x), 0, s).  With a known mother m the
 *     same from LP_m, LM_m with the T of (ID(x), 1, s).
 *   - Under selfing the two sides draw independent words.
 * Statistics.  For the pair (i, j) of listed probands in simulation s at locus k < L, take a = LP_i, b = LM_i, c = LP_j, d = LM_j:
 *   e = [a=c] + [a=d] + [b=c] + [b=d];  any = e > 0;  two = (a=c and b=d) or (a=d and b=c).
 * Per simulation: m_s = sum_k e; n1_s = sum_k any; n2_s = sum_k two; g_s = the number of maximal runs of consecutive loci with any
 * (runs do not wrap round, and loci >= L do not exist).  The result is sums[i, j, 0 .. 5], Int64, n_pro x n_pro x 6, row-major:
 *   0: sum_s m_s    1: sum_s m_s^2    2: sum_s n1_s    3: sum_s n2_s    4: sum_s g_s    5: sum_s [n1_s > 0]
 * All six are symmetric in (i, j).  m_s <= 4 L <= 2^14, so sum_s m_s^2 <= 2^52.
 * Labels.  Under GENPHI_LINK_FLAG_LABELS the result also carries the probands' labels, n_pro x 2 x S x L Int32.  They are refused
 * with GENPHI_ERR_ALLOC before any launch when they do not fit: by compute for the device at hand, and by create already when they
 * are 2^48 bytes or more.
 * Invariants, all exact.  The result is a pure function of (pedigree relations, proband IDs, L, q, seed, S): it does not depend
 * on the panel width or on ALL_PAIRS; a sub-list of probands gives the sub-block; gen.branching(ped, pro=P) first changes nothing;
 * the labels of S = 3 are the first three simulations of S = 100.  With q = 0 every locus of a simulation carries the same label,
 * so m_s is L times 0, 1, 2 or 4 and g_s = [n1_s > 0].  A diagonal pair has n1_s = L and g_s = 1.
 * Errors.  Those of genphi_ident_create; L or q out of range -> GENPHI_ERR_ARG.
 * Method.  ident's planes, with the column of a panel row running over (simulation, pair of words), the pair fastest.  In the step
 * kernel the lanes that own the pairs of words of one simulation are neighbours in a wave; each draws and folds its own X words,
 * and the parity of all earlier words reaches it by a segmented XOR scan over those lanes (wave shuffles); inside a word the prefix
 * is six shift-and-XOR steps.  The pair kernel has ident's tiles and walks simulation-major: per word the four equality words,
 * any and two, popcounts, and the runs as popcount(any & ~(any << 1 | carry)) with the carry from the previous word.
 *   create            host only (no GPU): ident's checks and plan.  A panel is a whole number of simulations: panel_sims of them, cut
 *                     to S; 0 = all of S, or the most that fit the device
 *   levels, alleles   as genphi_ident_levels and genphi_ident_alleles
 *   compute           the sweep on `device` (-1 = current); sums (and labels) stay resident
 *   sums_to_host      out: n_pro x n_pro x 6 Int64, row-major
 *   labels_to_host    out: n_pro x 2 x S x L Int32, row-major; GENPHI_ERR_ARG without GENPHI_LINK_FLAG_LABELS
 *   stats             of the last compute, by HIP events: the device time of init and level steps, and of gather and pair kernel,
 *                     summed over the panels; the algorithmic bytes of the steps (per side with a known parent and simulation: two
 *                     runs of B planes read and one written, 16 bytes per plane and pair of words); the word operations of the pair
 *                     kernel (pairs computed -- n_pro (n_pro + 1) / 2, or n_pro^2 under ALL_PAIRS -- x S x W x (8 B + 32): per plane
 *                     an XOR and an OR for each of the four equality words, then 8 to negate and mask them, 6 for any and two, 12
 *                     for the six popcounts and their adds and 6 for the run count and its carry); the Philox blocks drawn (per
 *                     side with a known parent and simulation: W x (8 - first block drawn) + 1); levels; the simulations of a
 *                     panel; the panels; B; the pair kernel's tile rows and columns; the lanes per simulation of the step kernel
 *   words             host only, as genphi_bootstrap_counts is: X[0 .. W) and T[0 .. W) of (seed, ID, side, simulation s) for L loci
 *                     at q, from the code the step kernel draws with; either may be NULL.  GENPHI_ERR_ARG: L, q, side or s (0 ..
 *                     2^24 - 1) out of range                                                                                       */
#define GENPHI_LINK_FLAG_LABELS 1
#define GENPHI_LINK_FLAG_ALL_PAIRS 2
#define GENPHI_LINK_MAX_LOCI 4096
#define GENPHI_LINK_MAX_Q 32768
typedef struct genphi_link genphi_link;
int genphi_link_create(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                       int64_t n_pro, const int64_t *pro_ids, int32_t loci, int32_t q, int64_t simul_no, uint64_t seed,
                       int32_t panel_sims, int32_t flags, genphi_link **out);
int genphi_link_levels(const genphi_link *h, int64_t *n_live, int32_t *levels, int64_t *rows_per_level);
int genphi_link_alleles(const genphi_link *h, int64_t *n_labels, int32_t *planes, int64_t *ids, int32_t *sides);
int genphi_link_compute(genphi_link *h, int32_t device);
int genphi_link_sums_to_host(genphi_link *h, int64_t *out);
int genphi_link_labels_to_host(genphi_link *h, int32_t *out);
int genphi_link_stats(const genphi_link *h, double *sweep_ms, double *pair_ms, double *algorithmic_bytes, double *word_ops,
                      double *philox_blocks, int32_t *levels, int32_t *panel_sims, int64_t *panels, int32_t *planes,
                      int32_t *tile_rows, int32_t *tile_cols, int32_t *lanes_per_sim);
void genphi_link_destroy(genphi_link *h);
int genphi_link_words(uint64_t seed, int64_t id, int32_t side, int64_t s, int32_t loci, int32_t q, uint64_t *X, uint64_t *T);

/* ---- gen.simuSegments: the lengths of the IBD segments of gen.simuSharing (csrc/link.hip, csrc/link.cpp, csrc/link_segments.h) ------
 * gen.simuSharing reduces the word `any` of a pair to the number of its runs (sums[.., 4]) and of its loci (sums[.., 2]); the lengths
 * of the runs are what a genealogy is compared with the segments that detection software reports, and they are kept here.  The
 * functions work on a genphi_link handle: a request is answered by the next genphi_link_compute, beside the sums.
 * Segment.  For a pair of list positions (i, j) in one simulation: a maximal run of consecutive loci with `any` set, the run that
 * g_s counts.  Its length is a number of loci, 1 .. L.
 * Censored.  A segment that contains locus 0 or locus L - 1: the chromosome cut it short.  A segment of length L is censored.
 * Edges.  n_edges strictly increasing Int32 with 1 <= edges[0], edges[n_edges - 1] <= 4097 and 2 <= n_edges <= 257; n_bins =
 * n_edges - 1.  A length len is in bin b when edges[b] <= len < edges[b + 1], in `below` when len < edges[0] and in `above` when
 * len >= edges[n_bins].  Lengths are integers: the last bin has no rule of its own.  (gen.simuSegments' default edges are 1, 2, 4, ..
 * up to and including the first power of two above L, the last one capped at 4097: at L = 4096 they end 2048, 4096, 4097.)
 * Histogram.  Over the unordered pairs i < j of list positions, never the diagonal.  hist[a][b][k][3], Int64, row-major: k = 0 is
 * `below`, k = 1 .. n_bins the bins, k = n_bins + 1 `above`; the three numbers of a cell are the segments, the loci in them and the
 * censored segments.  Without groups a = b = 0.  With groups, group[i] is the label of list position i, 0 .. n_groups - 1, or -1 for
 * "counts nowhere" (as in genphi_result_hist): a segment of the pair (i, j) counts in hist[group[i]][group[j]] and in its mirror;
 * the table is symmetric and hist[a][a] holds the pairs within group a.  n_groups <= 32, and with G = max(n_groups, 1) the cells
 * G (G + 1) / 2 x (n_bins + 2) are at most 2048.
 * Per pair.  pairs[i][j][3], Int64, n_pro x n_pro x 3, symmetric, the diagonal included: the sums over the simulations of the
 * segments with len >= min_loci, of the loci in those segments, and of the longest segment of the simulation (0 when it has none,
 * whatever min_loci is).  1 <= min_loci <= 4097.
 * Invariants, all exact.  Everything is an integer and is added by integer additions only: the result is a function of the pedigree's
 * relations, the list, L, q, the seed, S, the edges, min_loci and the labels, and does not depend on the panel width, the order of
 * the tiles or ALL_PAIRS.  Over i < j: the segments of all cells add up to sum g and their loci to sum n1.  With min_loci = 1,
 * pairs[.., 0] = sums[.., 4] and pairs[.., 1] = sums[.., 2].
 * Method.  A second kernel after the pair kernel, on the same gathered rows, with the pair kernel's tile and staging; it forms the
 * four equality words and `any`, and walks the runs of `any` with a state carried from word to word of a simulation (the length of
 * the open run, whether it began at locus 0, the longest so far): a zero word with nothing open and a full word are one step, else
 * the runs are peeled with count-trailing-zeros on the word and its complement.  A closed run goes to the thread's Int64 of the pair
 * and, for i < j, to the workgroup's table in LDS (64-bit counters), which is added to the global table once at the end by 64-bit
 * integer atomics.
 *   request      takes effect at the next genphi_link_compute; n_edges = 0 withdraws the request.  Everything is checked on the host:
 *                GENPHI_ERR_ARG with a message that names the offending value; the handle, an earlier request and earlier results
 *                stay as they were.  group is read only with n_groups > 0: n_pro labels
 *   to_host      hist: G x G x (n_bins + 2) x 3 Int64, mirrored here; pairs: n_pro x n_pro x 3 Int64; either may be NULL.
 *                GENPHI_ERR_ARG unless the last compute succeeded and ran with a request (a compute that fails leaves no result,
 *                the segments included)
 *   stats        of the last compute: the device time of the segment kernel by HIP events, summed over the panels; its word
 *                operations (pairs walked x S x W x (8 B + 10): the equality words as in the pair kernel, 8 to negate and mask, 3
 *                for any, and the two tests of the walk's common words; the peeled runs are not counted); the segments closed,
 *                summed from the table; the cells of the request; the dynamic LDS of a workgroup in bytes
 *   host         host only, in the role of genphi_link_words: one pair and one simulation, the chromosome's `any` given as
 *                ceil(loci / 64) words (bits at and above loci are ignored), reduced by the code the kernel walks with.  hist_out:
 *                (n_bins + 2) x 3, pair_out: 3; both are added to, either may be NULL                                            */
#define GENPHI_SEG_MAX_EDGES 257
#define GENPHI_SEG_MAX_EDGE 4097
#define GENPHI_SEG_MAX_GROUPS 32
#define GENPHI_SEG_MAX_CELLS 2048
int genphi_seg_request(genphi_link *h, int32_t n_edges, const int32_t *edges, int32_t min_loci, int32_t n_groups, const int32_t *group);
int genphi_seg_to_host(genphi_link *h, int64_t *hist, int64_t *pairs);
int genphi_seg_stats(const genphi_link *h, double *segment_ms, double *word_ops, int64_t *segments, int32_t *cells, int64_t *lds_bytes);
int genphi_seg_host(int32_t loci, const uint64_t *any_words, int32_t n_edges, const int32_t *edges, int32_t min_loci, int64_t *hist_out,
                    int64_t *pair_out);

/* gen.descendant and gen.children (src/identify.jl:203-215, :77-80), host only: the strict descendants of ids[0 .. n_ids) (the
 * union over them), and the children of one ID, ascending; *out is allocated by the library (genphi_free).  No order of the
 * pedigree is assumed.  Unknown ID -> GENPHI_ERR_UNKNOWN_ID.                                                                  */
int genphi_descendants(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_ids,
                       const int64_t *ids, int64_t *n_out, int64_t **out);
int genphi_children(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t id, int64_t *n_out,
                    int64_t **out);

/* Frees host and device memory of the plan (NULL is allowed). */
void genphi_plan_destroy(genphi_plan *plan);

/* Message of the last error on this thread ("" if none). */
const char *genphi_last_error(void);

/* Library version string. */
const char *genphi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GENPHI_H */
