/*
 * slot_oracle.cpp -- a second CPU restatement of GenLib.jl's sparse_phi / KinshipMatrix whose memory is
 * bounded by the live set instead of by the reference's dictionaries.
 *
 * TEST INFRASTRUCTURE ONLY.  Only tests/ may load this library (through oracle/oracle.py: SlotSparsePhi).
 *
 * Same semantics as oracle/sparse_oracle.cpp (src/compute.jl:321-447, :31-46, :467-472), other containers:
 *   - the queue is walked literally, one individual at a time (a deque, founders by ascending ID, a child
 *     enqueued once both its parents are done, children_to_process counted down); no depths, no waves;
 *   - every live individual owns a slot of a dense (peak live) x (peak live) Float32 matrix, symmetric, whose
 *     (a, b) element is the value the reference stores under the key (earlier processed, later processed)
 *     of the two owners, 0 where it stores nothing.  A slot is reused once its owner retires;
 *   - a lookup under (smaller rank, larger rank) finds the stored value only if the earlier processed one
 *     has the smaller rank (the self entry is always found), exactly the reference's key rule;
 *   - a non-proband x that retires (src/compute.jl:401-430) leaves behind, in the dictionary of every live
 *     proband j processed before it with rank_j > rank_x, the entry (rank_j, rank_x) if it is > 0: those
 *     are appended to a list.  Entries held by non-probands vanish when they retire, as in the reference.
 * At the end the live set is exactly the probands; their block is kept, the big matrix is freed.
 *
 * One row of the matrix per new individual is computed in parallel over the live set (OpenMP); each value is
 * RN32(Float64 sum of the two Float32 halves), as src/compute.jl:363-394 computes it.
 */
#include <algorithm>
#include <cstdint>
#include <deque>
#include <memory>
#include <new>
#include <unordered_map>
#include <vector>

#include <omp.h>

namespace {

struct Slots {
    int64_t n_pro = 0;                         /* distinct probands */
    std::unordered_map<int64_t, int> pos;      /* proband ID -> position in the block */
    std::vector<int> rank, proc;               /* per position: rank (1-based), processing index */
    std::vector<float> block;                  /* n_pro x n_pro, symmetric, by position */
    std::vector<int> stale_row, stale_col;     /* entries that outlive their column: (proband rank, retired rank, value) */
    std::vector<float> stale_val;
    int64_t peak_live = 0;
};

}  // namespace

extern "C" {

/* ped arrays in rank order (parents before children), 0 = unknown parent.  *rc: 0, 1 = unknown proband ID,
 * 2 = an individual is its own father and mother (not supported), 3 = out of memory. */
void *slot_oracle_create(int64_t n, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                         const int64_t *pro, int n_threads, int *rc)
{
    *rc = 0;
    std::unordered_map<int64_t, int> at;
    at.reserve(static_cast<size_t>(n) * 2);
    for (int64_t i = 0; i < n; ++i) at[ind[i]] = static_cast<int>(i);
    /* branching(pedigree, pro = probandIDs): the probands' ancestors, in pedigree order, ranks 1.. in that order */
    std::vector<char> keep(n, 0);
    std::vector<int> stack;
    for (int64_t k = 0; k < n_pro; ++k) {
        auto it = at.find(pro[k]);
        if (it == at.end()) { *rc = 1; return nullptr; }
        stack.push_back(it->second);
        while (!stack.empty()) {
            const int x = stack.back(); stack.pop_back();
            if (keep[x]) continue;
            keep[x] = 1;
            if (father[x] != 0) stack.push_back(at[father[x]]);
            if (mother[x] != 0) stack.push_back(at[mother[x]]);
        }
    }
    std::vector<int> iso_of(n, -1), fa, mo;                 /* isolated pedigree: index = rank - 1 */
    std::vector<int64_t> id;
    for (int64_t i = 0; i < n; ++i) {
        if (!keep[i]) continue;
        iso_of[i] = static_cast<int>(id.size());
        id.push_back(ind[i]);
        fa.push_back(father[i] != 0 ? iso_of[at[father[i]]] : -1);
        mo.push_back(mother[i] != 0 ? iso_of[at[mother[i]]] : -1);
        if (fa.back() >= 0 && fa.back() == mo.back()) { *rc = 2; return nullptr; }
    }
    const int m = static_cast<int>(id.size());
    std::vector<std::vector<int>> children(m);              /* in pedigree order */
    for (int u = 0; u < m; ++u) {
        if (fa[u] >= 0) children[fa[u]].push_back(u);
        if (mo[u] >= 0) children[mo[u]].push_back(u);
    }
    std::vector<char> is_pro(m, 0);
    for (int64_t k = 0; k < n_pro; ++k) is_pro[iso_of[at[pro[k]]]] = 1;

    /* ---- the queue, literally: processing order, and who retires after each processing step ---- */
    std::vector<int> order, proc(m, -1), to_process(m, 0);
    std::vector<int> retire_after_first(m, -1), retire_after_second(m, -1);   /* by processing index */
    {
        std::deque<int> queue;
        std::vector<std::pair<int64_t, int>> f;
        for (int u = 0; u < m; ++u)
            if (fa[u] < 0 && mo[u] < 0) f.emplace_back(id[u], u);
        std::sort(f.begin(), f.end());                      /* founder(): IDs ascending */
        for (auto &e : f) queue.push_back(e.second);
        std::vector<char> done(m, 0);
        while (!queue.empty()) {
            const int u = queue.front(); queue.pop_front();
            const int k = static_cast<int>(order.size());
            order.push_back(u);
            proc[u] = k;
            done[u] = 1;
            to_process[u] = static_cast<int>(children[u].size());
            for (int side = 0; side < 2; ++side) {
                const int p = side == 0 ? fa[u] : mo[u];
                if (p < 0 || is_pro[p]) continue;
                if (--to_process[p] == 0) (side == 0 ? retire_after_first : retire_after_second)[k] = p;
            }
            for (int c : children[u]) {
                if (fa[c] >= 0 && mo[c] >= 0) {
                    if (done[fa[c]] && done[mo[c]]) queue.push_back(c);
                } else {
                    queue.push_back(c);
                }
            }
        }
    }
    /* the peak live set sizes the matrix */
    int64_t live = 0, peak = 0;
    for (size_t k = 0; k < order.size(); ++k) {
        peak = std::max(peak, ++live);
        live -= (retire_after_first[k] >= 0) + (retire_after_second[k] >= 0);
    }
    const size_t D = static_cast<size_t>(peak);
    std::unique_ptr<float[]> M(new (std::nothrow) float[std::max<size_t>(1, D * D)]);   /* (no zero fill: a slot's row and column
                                                                                              are written for every live partner
                                                                                              before they are read) */
    if (!M) { *rc = 3; return nullptr; }
    Slots *S = new Slots();
    S->peak_live = peak;

    std::vector<int> slot(m, -1), free_slots, live_slots, live_at(D, -1), owner(D, -1), live_pro;
    int next_slot = 0;
    auto found = [&](int a, int b) { return a == b || ((proc[a] < proc[b]) == (a < b)); };   /* rank order = index order */
    if (n_threads > 0) omp_set_num_threads(n_threads);
    for (size_t k = 0; k < order.size(); ++k) {
        const int u = order[k];
        int s;
        if (!free_slots.empty()) { s = free_slots.back(); free_slots.pop_back(); } else s = next_slot++;
        slot[u] = s; owner[s] = u;
        float *row = M.get() + static_cast<size_t>(s) * D;
        const int f = fa[u], mth = mo[u];
        const int sf = f >= 0 ? slot[f] : -1, sm = mth >= 0 ? slot[mth] : -1;
        /* kinship with self, src/compute.jl:349-361 */
        double self = 0.5;
        if (f >= 0 && mth >= 0 && found(f, mth)) self += static_cast<double>(M[static_cast<size_t>(sf) * D + sm] / 2.0f);
        /* kinship with every live individual, :363-395 */
        const int nl = static_cast<int>(live_slots.size());
        const int *ls = live_slots.data();
        float *Mp = M.get();
#pragma omp parallel for schedule(static) if (nl > 2048)
        for (int t = 0; t < nl; ++t) {
            const int sj = ls[t], j = owner[sj];
            double c = 0.0;
            if (f >= 0 && found(f, j)) c += static_cast<double>(Mp[static_cast<size_t>(sf) * D + sj] / 2.0f);
            if (mth >= 0 && found(mth, j)) c += static_cast<double>(Mp[static_cast<size_t>(sm) * D + sj] / 2.0f);
            const float v = c > 0.0 ? static_cast<float>(c) : 0.0f;
            row[sj] = v;
            Mp[static_cast<size_t>(sj) * D + s] = v;
        }
        row[s] = static_cast<float>(self);
        live_at[s] = static_cast<int>(live_slots.size());
        live_slots.push_back(s);
        if (is_pro[u]) live_pro.push_back(s);
        /* retirement of parents whose children are all processed, :401-430 */
        for (int r : {retire_after_first[k], retire_after_second[k]}) {
            if (r < 0) continue;
            const int sr = slot[r];
            for (int sj : live_pro) {                        /* the entries of the retired column that probands keep */
                const int j = owner[sj];
                const float v = M[static_cast<size_t>(sj) * D + sr];
                if (proc[j] < proc[r] && j > r && v > 0.0f) {
                    S->stale_row.push_back(j + 1); S->stale_col.push_back(r + 1); S->stale_val.push_back(v);
                }
            }
            const int at_r = live_at[sr], last = live_slots.back();
            live_slots[at_r] = last; live_at[last] = at_r; live_slots.pop_back();
            live_at[sr] = -1; owner[sr] = -1;
            free_slots.push_back(sr);
        }
    }
    /* the final live set is the probands: their block, by position in the (deduplicated) proband list */
    for (int64_t k = 0; k < n_pro; ++k) {
        if (S->pos.count(pro[k])) continue;
        const int u = iso_of[at[pro[k]]];
        S->pos[pro[k]] = static_cast<int>(S->rank.size());
        S->rank.push_back(u + 1);
        S->proc.push_back(proc[u]);
    }
    const int64_t N = static_cast<int64_t>(S->rank.size());
    S->n_pro = N;
    S->block.resize(static_cast<size_t>(N * N));
    for (int64_t a = 0; a < N; ++a)
        for (int64_t b = 0; b < N; ++b)
            S->block[a * N + b] = M[static_cast<size_t>(slot[S->rank[a] - 1]) * D + slot[S->rank[b] - 1]];
    return S;
}

void slot_oracle_free(void *h) { delete static_cast<Slots *>(h); }

int64_t slot_oracle_peak_live(void *h) { return static_cast<Slots *>(h)->peak_live; }

/* getindex(ϕ, id1[k], id2[k]) for k < n (src/compute.jl:36-40): looked up under (smaller rank, larger rank).  Returns the first k
 * whose IDs are not both probands, or -1. */
int64_t slot_oracle_get(void *h, int64_t n, const int64_t *id1, const int64_t *id2, float *out)
{
    const Slots *S = static_cast<Slots *>(h);
    for (int64_t k = 0; k < n; ++k) {
        auto a = S->pos.find(id1[k]), b = S->pos.find(id2[k]);
        if (a == S->pos.end() || b == S->pos.end()) return k;
        const int pa = a->second, pb = b->second;
        const bool hit = pa == pb || ((S->proc[pa] < S->proc[pb]) == (S->rank[pa] < S->rank[pb]));
        out[k] = hit ? S->block[static_cast<size_t>(pa) * S->n_pro + pb] : 0.0f;
    }
    return -1;
}

/* what `show` prints (:42-46) and the sums phiMean uses (:467-472), in Float64 */
void slot_oracle_info(void *h, int64_t *n_rows, int64_t *n_stored, double *sum_all, double *sum_diag)
{
    const Slots *S = static_cast<Slots *>(h);
    const int64_t N = S->n_pro;
    int64_t nz = 0;
    double tot = 0.0, dg = 0.0;
    for (int64_t a = 0; a < N; ++a) {
        const float self = S->block[a * N + a];
        nz += 1; tot += self; dg += self;
        for (int64_t b = a + 1; b < N; ++b) {
            const float v = S->block[a * N + b];
            if (v > 0.0f) { nz += 1; tot += v; }            /* one key per pair of probands, stored when > 0 */
        }
    }
    for (float v : S->stale_val) { nz += 1; tot += v; }
    *n_rows = N; *n_stored = nz; *sum_all = tot; *sum_diag = dg;
}

/* every stored entry as (row rank, column rank, value) under the reference's key (earlier processed, later processed); returns
 * the count, fills at most cap */
int64_t slot_oracle_entries(void *h, int64_t cap, int64_t *row_rank, int64_t *col_rank, float *val)
{
    const Slots *S = static_cast<Slots *>(h);
    const int64_t N = S->n_pro;
    int64_t k = 0;
    auto put = [&](int64_t r, int64_t c, float v) { if (k < cap) { row_rank[k] = r; col_rank[k] = c; val[k] = v; } ++k; };
    for (int64_t a = 0; a < N; ++a)
        for (int64_t b = 0; b < N; ++b) {
            const float v = S->block[a * N + b];
            if (a == b) put(S->rank[a], S->rank[a], v);
            else if (S->proc[a] < S->proc[b] && v > 0.0f) put(S->rank[a], S->rank[b], v);
        }
    for (size_t t = 0; t < S->stale_val.size(); ++t) put(S->stale_row[t], S->stale_col[t], S->stale_val[t]);
    return k;
}

}  // extern "C"
