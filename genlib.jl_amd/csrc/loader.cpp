// loader.cpp -- native pedigree loader and pruning: the steps BEFORE the gen.phi hot path
// (genealogy(filename) and branching).
//
// Replaces, for callers that want it, the reference's genealogy(filename; sort)
// (src/create.jl:161-189: header line skipped, four whitespace-separated Ints per row) followed
// by _ordered_pedigree (src/create.jl:196-227: stable sort by maximum ancestral depth, founders
// depth 1).  The output is exactly what genphi_plan_create wants: ind / father / mother (/ sex)
// in rank order.  Own design: one pass over a memory-resident buffer with a hand-rolled integer
// scanner, iterative depth computation (no recursion: depth-1e6 chains are fine), counting sort.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/genphi.h"
#include "error.h"

namespace {

struct Cols { std::vector<int64_t> ind, father, mother, sex; };

// ID -> position for the searches below: a direct table when the IDs are non-negative and dense enough, else a hash map; -1 =
// unknown.  Of a duplicated ID the last position counts.
struct IdIndex {
    std::vector<int32_t> table;
    std::unordered_map<int64_t, int32_t> map;
    bool direct = false;
    void init(int64_t n, const int64_t *ind)
    {
        int64_t lo = INT64_MAX, hi = INT64_MIN;
        for (int64_t i = 0; i < n; ++i) { lo = std::min(lo, ind[i]); hi = std::max(hi, ind[i]); }
        direct = n > 0 && lo >= 0 && hi < 3 * n + 1024;
        if (direct) {
            table.assign(static_cast<size_t>(hi) + 1, -1);
            for (int64_t i = 0; i < n; ++i) table[ind[i]] = static_cast<int32_t>(i);
        } else {
            map.reserve(static_cast<size_t>(n) * 2);
            for (int64_t i = 0; i < n; ++i) map[ind[i]] = static_cast<int32_t>(i);
        }
    }
    int32_t find(int64_t id) const
    {
        if (direct) return (id < 0 || id >= static_cast<int64_t>(table.size())) ? -1 : table[id];
        auto it = map.find(id);
        return it == map.end() ? -1 : it->second;
    }
};

bool parse_tsv(const char *buf, size_t len, Cols &c, std::string &err)
{
    size_t i = 0;
    while (i < len && buf[i] != '\n') ++i;          // header row
    if (i < len) ++i;
    size_t line = 1;
    while (i < len) {
        ++line;
        int64_t v[4];
        int got = 0;
        while (i < len && buf[i] != '\n') {
            while (i < len && (buf[i] == ' ' || buf[i] == '\t' || buf[i] == '\r')) ++i;
            if (i >= len || buf[i] == '\n') break;
            bool neg = false;
            if (buf[i] == '-' || buf[i] == '+') { neg = buf[i] == '-'; ++i; }
            if (i >= len || buf[i] < '0' || buf[i] > '9') { err = "line " + std::to_string(line) + ": not an integer"; return false; }
            int64_t x = 0;
            while (i < len && buf[i] >= '0' && buf[i] <= '9') { x = x * 10 + (buf[i] - '0'); ++i; }
            if (got < 4) v[got] = neg ? -x : x;
            ++got;
        }
        if (i < len) ++i;                            // newline
        if (got == 0) continue;                      // blank line
        if (got != 4) { err = "line " + std::to_string(line) + ": expected 4 columns (ind father mother sex), got " + std::to_string(got); return false; }
        c.ind.push_back(v[0]); c.father.push_back(v[1]); c.mother.push_back(v[2]); c.sex.push_back(v[3]);
    }
    return true;
}

// depth(x) = 1 + max(depth(father), depth(mother)) (founders 1) from the parents' positions (-1 = unknown); explicit stack (no
// recursion: depth-1e6 chains are fine); false: the pedigree contains a cycle
bool ancestral_depths(const std::vector<int32_t> &pf, const std::vector<int32_t> &pm, std::vector<int32_t> &depth)
{
    const int64_t n = static_cast<int64_t>(pf.size());
    depth.assign(n, 0);
    std::vector<int32_t> state(n, 0), stack;
    for (int64_t s0 = 0; s0 < n; ++s0) {
        if (depth[s0]) continue;
        stack.push_back(static_cast<int32_t>(s0));
        while (!stack.empty()) {
            const int32_t x = stack.back();
            const int32_t f = pf[x], m = pm[x];
            state[x] = 1;
            if (f >= 0 && !depth[f]) { if (state[f]) return false; stack.push_back(f); continue; }
            if (m >= 0 && !depth[m]) { if (state[m]) return false; stack.push_back(m); continue; }
            const int32_t fd = f >= 0 ? depth[f] : 0, md = m >= 0 ? depth[m] : 0;
            depth[x] = (fd > md ? fd : md) + 1;
            stack.pop_back();
        }
    }
    return true;
}

}  // namespace

// Everything after the table is in memory: ID lookup, checks, depth sort (src/create.jl:196-254), output arrays in rank order.
static int order_and_emit(const Cols &c, int32_t sort, int64_t *n_out, int64_t **ind_out, int64_t **father_out, int64_t **mother_out,
                          int64_t **sex_out)
{
    const int64_t n = static_cast<int64_t>(c.ind.size());

    // file position of every id; parents must exist (KeyError in the reference).  IDs in a moderate range go through a direct table
    // (1e6 dense IDs: 10 ms instead of 150 ms of hashing), anything else through a hash map.
    std::vector<int32_t> table;
    std::unordered_map<int64_t, int32_t> pos;
    bool direct = false;
    {
        int64_t lo = INT64_MAX, hi = INT64_MIN;
        for (int64_t i = 0; i < n; ++i) { lo = c.ind[i] < lo ? c.ind[i] : lo; hi = c.ind[i] > hi ? c.ind[i] : hi; }
        if (n > 0 && lo >= 0 && hi < 64 * n + (1 << 20)) { table.assign(static_cast<size_t>(hi) + 1, -1); direct = true; }
        else pos.reserve(static_cast<size_t>(n) * 2);
    }
    auto find = [&](int64_t id) -> int32_t {
        if (direct) return (id < 0 || id >= static_cast<int64_t>(table.size())) ? -1 : table[id];
        auto it = pos.find(id);
        return it == pos.end() ? -1 : it->second;
    };
    for (int64_t i = 0; i < n; ++i) {
        bool fresh;
        if (direct) { fresh = table[c.ind[i]] < 0; if (fresh) table[c.ind[i]] = static_cast<int32_t>(i); }
        else fresh = pos.emplace(c.ind[i], static_cast<int32_t>(i)).second;
        if (!fresh) return genphi_set_error(GENPHI_ERR_DUPLICATE_ID, "duplicate individual ID " + std::to_string(c.ind[i]));
    }
    std::vector<int32_t> pf(n, -1), pm(n, -1);
    for (int64_t i = 0; i < n; ++i) {
        if (c.father[i] != 0) {
            pf[i] = find(c.father[i]);
            if (pf[i] < 0) return genphi_set_error(GENPHI_ERR_UNKNOWN_ID, "KeyError: father " + std::to_string(c.father[i]) + " of " + std::to_string(c.ind[i]) + " not found");
        }
        if (c.mother[i] != 0) {
            pm[i] = find(c.mother[i]);
            if (pm[i] < 0) return genphi_set_error(GENPHI_ERR_UNKNOWN_ID, "KeyError: mother " + std::to_string(c.mother[i]) + " of " + std::to_string(c.ind[i]) + " not found");
        }
    }
    std::vector<int64_t> order(n);
    if (sort) {
        std::vector<int32_t> depth;
        if (!ancestral_depths(pf, pm, depth)) return genphi_set_error(GENPHI_ERR_ARG, "pedigree contains a cycle");
        int32_t maxd = 0;
        for (int64_t i = 0; i < n; ++i) maxd = depth[i] > maxd ? depth[i] : maxd;
        std::vector<int64_t> cnt(static_cast<size_t>(maxd) + 2, 0);
        for (int64_t i = 0; i < n; ++i) cnt[depth[i] + 1]++;
        for (int32_t d = 1; d <= maxd + 1; ++d) cnt[d] += cnt[d - 1];
        for (int64_t i = 0; i < n; ++i) order[cnt[depth[i]]++] = i;         // stable: file order on ties
    } else {
        for (int64_t i = 0; i < n; ++i) {
            order[i] = i;
            if ((pf[i] >= 0 && pf[i] >= i) || (pm[i] >= 0 && pm[i] >= i))
                return genphi_set_error(GENPHI_ERR_ORDER, "KeyError: a parent of " + std::to_string(c.ind[i]) + " is listed after it (sort=false)");
        }
    }
    auto emit = [&](const std::vector<int64_t> &src) -> int64_t * {
        int64_t *dst = static_cast<int64_t *>(std::malloc(sizeof(int64_t) * static_cast<size_t>(n > 0 ? n : 1)));
        if (dst) for (int64_t k = 0; k < n; ++k) dst[k] = src[order[k]];
        return dst;
    };
    int64_t *a = emit(c.ind), *b = emit(c.father), *d = emit(c.mother), *e = (sex_out && c.sex.size() == c.ind.size()) ? emit(c.sex) : nullptr;
    if (!a || !b || !d || (sex_out && c.sex.size() == c.ind.size() && !e)) { std::free(a); std::free(b); std::free(d); std::free(e); return genphi_set_error(GENPHI_ERR_ALLOC, "out of memory"); }
    *n_out = n; *ind_out = a; *father_out = b; *mother_out = d;
    if (sex_out) *sex_out = e;
    return GENPHI_OK;
}


extern "C" {

void genphi_free(void *ptr) { std::free(ptr); }

int genphi_genealogy_read(const char *path, int32_t sort, int64_t *n_out, int64_t **ind_out, int64_t **father_out,
                          int64_t **mother_out, int64_t **sex_out)
{
    if (!path || !n_out || !ind_out || !father_out || !mother_out) return genphi_set_error(GENPHI_ERR_ARG, "genphi_genealogy_read: NULL argument");
    *n_out = 0; *ind_out = *father_out = *mother_out = nullptr;
    if (sex_out) *sex_out = nullptr;
    std::FILE *fh = std::fopen(path, "rb");
    if (!fh) return genphi_set_error(GENPHI_ERR_ARG, std::string("cannot open ") + path);
    std::string buf;
    {
        std::fseek(fh, 0, SEEK_END);
        const long sz = std::ftell(fh);
        std::fseek(fh, 0, SEEK_SET);
        buf.resize(sz > 0 ? static_cast<size_t>(sz) : 0);
        const size_t rd = buf.empty() ? 0 : std::fread(&buf[0], 1, buf.size(), fh);
        std::fclose(fh);
        if (rd != buf.size()) return genphi_set_error(GENPHI_ERR_ARG, std::string("short read on ") + path);
    }
    Cols c;
    std::string err;
    if (!parse_tsv(buf.data(), buf.size(), c, err)) return genphi_set_error(GENPHI_ERR_ARG, std::string(path) + ": " + err);
    return order_and_emit(c, sort, n_out, ind_out, father_out, mother_out, sex_out);
}

/* The same for a table already in memory (gen.genealogy(dataframe; sort), src/create.jl:131-146 + :196-254): ind / father / mother
 * (/ sex, may be NULL) in file order -> rank order.  Errors as genphi_genealogy_read: duplicate ID, unknown parent (KeyError in the
 * reference), a cycle, and with sort = 0 a parent listed after its child (KeyError). */
int genphi_genealogy_order(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, const int64_t *sex, int32_t sort,
                           int64_t *n_out, int64_t **ind_out, int64_t **father_out, int64_t **mother_out, int64_t **sex_out)
{
    if (n_ind < 0 || (n_ind > 0 && (!ind || !father || !mother)) || !n_out || !ind_out || !father_out || !mother_out)
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_genealogy_order: NULL or negative argument");
    *n_out = 0; *ind_out = *father_out = *mother_out = nullptr;
    if (sex_out) *sex_out = nullptr;
    Cols c;
    c.ind.assign(ind, ind + n_ind); c.father.assign(father, father + n_ind); c.mother.assign(mother, mother + n_ind);
    if (sex) c.sex.assign(sex, sex + n_ind);
    return order_and_emit(c, sort, n_out, ind_out, father_out, mother_out, sex_out);
}

// gen.branching (src/extract.jl:65-186).  The reference marks ancestors / descendants with two
// recursive walks over a pointer graph; here the pedigree is already in rank order (parents
// before children), so both marks are single linear passes: ancestors in one reverse sweep
// (a marked child marks its parents), descendants in one forward sweep (a marked parent marks
// its children).  No recursion, no per-individual allocation, O(N).
int genphi_branching(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                     const int64_t *sex, int64_t n_pro, const int64_t *pro, int64_t n_anc,
                     const int64_t *ancestors, int64_t *n_out, int64_t **ind_out, int64_t **father_out,
                     int64_t **mother_out, int64_t **sex_out)
{
    if (!n_out || !ind_out || !father_out || !mother_out || n_ind < 0 || (n_ind > 0 && (!ind || !father || !mother)) ||
        n_pro < 0 || n_anc < 0)
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_branching: bad argument");
    *n_out = 0; *ind_out = *father_out = *mother_out = nullptr;
    if (sex_out) *sex_out = nullptr;
    const int64_t n = n_ind;
    std::unordered_map<int64_t, int64_t> pos;
    pos.reserve(static_cast<size_t>(n) * 2);
    for (int64_t i = 0; i < n; ++i)
        if (!pos.emplace(ind[i], i).second)
            return genphi_set_error(GENPHI_ERR_DUPLICATE_ID, "duplicate individual ID " + std::to_string(ind[i]));
    std::vector<int64_t> pf(n, -1), pm(n, -1);
    for (int64_t i = 0; i < n; ++i) {
        for (int side = 0; side < 2; ++side) {
            const int64_t pid = side ? mother[i] : father[i];
            if (pid == 0) continue;
            auto it = pos.find(pid);
            if (it == pos.end()) return genphi_set_error(GENPHI_ERR_UNKNOWN_ID, "KeyError: parent " + std::to_string(pid) + " of " + std::to_string(ind[i]) + " not found");
            if (it->second >= i) return genphi_set_error(GENPHI_ERR_ORDER, "KeyError: a parent of " + std::to_string(ind[i]) + " is listed after it");
            (side ? pm : pf)[i] = it->second;
        }
    }
    std::vector<uint8_t> is_anc(n, 0), is_desc(n, 0);
    if (pro) {
        for (int64_t k = 0; k < n_pro; ++k) {
            auto it = pos.find(pro[k]);
            if (it == pos.end()) return genphi_set_error(GENPHI_ERR_UNKNOWN_ID, "KeyError: proband " + std::to_string(pro[k]) + " not found");
            is_anc[it->second] = 1;
        }
        for (int64_t i = n - 1; i >= 0; --i)
            if (is_anc[i]) {
                if (pf[i] >= 0) is_anc[pf[i]] = 1;
                if (pm[i] >= 0) is_anc[pm[i]] = 1;
            }
    }
    if (ancestors) {
        for (int64_t k = 0; k < n_anc; ++k) {
            auto it = pos.find(ancestors[k]);
            if (it == pos.end()) return genphi_set_error(GENPHI_ERR_UNKNOWN_ID, "KeyError: ancestor " + std::to_string(ancestors[k]) + " not found");
            is_desc[it->second] = 1;
        }
        for (int64_t i = 0; i < n; ++i)
            if (!is_desc[i] && ((pf[i] >= 0 && is_desc[pf[i]]) || (pm[i] >= 0 && is_desc[pm[i]]))) is_desc[i] = 1;
    }
    // kept set; a parent outside it becomes unknown (only possible when `ancestors` is given)
    std::vector<uint8_t> keep(n, 0);
    int64_t m = 0;
    for (int64_t i = 0; i < n; ++i) {
        keep[i] = (pro && ancestors) ? (is_anc[i] && is_desc[i]) : (pro ? is_anc[i] : (ancestors ? is_desc[i] : 0));
        m += keep[i];
    }
    const size_t bytes = sizeof(int64_t) * static_cast<size_t>(m > 0 ? m : 1);
    int64_t *a = static_cast<int64_t *>(std::malloc(bytes)), *b = static_cast<int64_t *>(std::malloc(bytes));
    int64_t *d = static_cast<int64_t *>(std::malloc(bytes)), *e = sex_out ? static_cast<int64_t *>(std::malloc(bytes)) : nullptr;
    if (!a || !b || !d || (sex_out && !e)) { std::free(a); std::free(b); std::free(d); std::free(e); return genphi_set_error(GENPHI_ERR_ALLOC, "out of memory"); }
    int64_t o = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (!keep[i]) continue;
        a[o] = ind[i];
        b[o] = (pf[i] >= 0 && keep[pf[i]]) ? father[i] : 0;
        d[o] = (pm[i] >= 0 && keep[pm[i]]) ? mother[i] : 0;
        if (e) e[o] = sex ? sex[i] : 0;
        ++o;
    }
    *n_out = m; *ind_out = a; *father_out = b; *mother_out = d;
    if (sex_out) *sex_out = e;
    return GENPHI_OK;
}

// gen.depth (src/describe.jl:43-66): the reference calls the un-memoised _max_depth for every individual -- every ascending path
// of every individual is walked.  Here: the depth pass of the loader's sort, once, and a maximum.  leaves_only: the maximum over the
// individuals without children (what Base.show(::Pedigree) prints, src/create.jl:76-111).  No arithmetic worth a launch: host only.
int genphi_genealogy_depth(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t *depth_out,
                           int32_t leaves_only)
{
    if (!depth_out || n_ind < 0 || n_ind >= INT32_MAX || (n_ind > 0 && (!ind || !father || !mother)))
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_genealogy_depth: bad argument");
    *depth_out = 0;
    IdIndex pos;
    pos.init(n_ind, ind);
    std::vector<int32_t> pf(n_ind, -1), pm(n_ind, -1);
    std::vector<uint8_t> has_child(n_ind, 0);
    for (int64_t i = 0; i < n_ind; ++i)
        for (int side = 0; side < 2; ++side) {
            const int64_t pid = side ? mother[i] : father[i];
            if (pid == 0) continue;
            const int32_t r = pos.find(pid);
            if (r < 0)
                return genphi_set_error(GENPHI_ERR_UNKNOWN_ID, "KeyError: parent " + std::to_string(pid) + " of " + std::to_string(ind[i]) + " not found");
            (side ? pm : pf)[i] = r;
            has_child[r] = 1;
        }
    std::vector<int32_t> depth;
    if (!ancestral_depths(pf, pm, depth)) return genphi_set_error(GENPHI_ERR_ARG, "pedigree contains a cycle");
    int32_t maxd = 0;
    for (int64_t i = 0; i < n_ind; ++i)
        if (!(leaves_only && has_child[i]) && depth[i] > maxd) maxd = depth[i];
    *depth_out = maxd;
    return GENPHI_OK;
}

// gen.ancestor (src/identify.jl:164-199): the strict ancestors of one ID, or the union over several, ascending.  The reference
// searches a pointer graph with a stack and a Set per call; here the same stack search runs on positions with one visited flag
// per individual.  No order of the pedigree is assumed.  *out is allocated by the library (genphi_free).
int genphi_ancestors(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_ids, const int64_t *ids,
                     int64_t *n_out, int64_t **out)
{
    if (!n_out || !out || n_ind < 0 || n_ids < 0 || (n_ind > 0 && (!ind || !father || !mother)) || (n_ids > 0 && !ids))
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_ancestors: bad argument");
    *n_out = 0; *out = nullptr;
    IdIndex pos;                                     // (a direct table for dense IDs: no hashing on the search path)
    pos.init(n_ind, ind);
    std::vector<uint8_t> seen(n_ind, 0);
    std::vector<int64_t> stack, found;
    for (int64_t k = 0; k < n_ids; ++k) {
        const int32_t r = pos.find(ids[k]);
        if (r < 0) return genphi_set_error(GENPHI_ERR_UNKNOWN_ID, "KeyError: individual " + std::to_string(ids[k]) + " not found");
        stack.push_back(r);                          // (an ID is not its own ancestor: it is searched, not flagged)
    }
    while (!stack.empty()) {
        const int64_t i = stack.back();
        stack.pop_back();
        for (int side = 0; side < 2; ++side) {
            const int64_t pid = side ? mother[i] : father[i];
            if (pid == 0) continue;
            const int32_t r = pos.find(pid);
            if (r < 0)
                return genphi_set_error(GENPHI_ERR_UNKNOWN_ID, "KeyError: parent " + std::to_string(pid) + " of " + std::to_string(ind[i]) + " not found");
            if (seen[r]) continue;                   // its ancestors are on the stack or done
            seen[r] = 1;
            found.push_back(pid);
            stack.push_back(r);
        }
    }
    std::sort(found.begin(), found.end());
    int64_t *a = static_cast<int64_t *>(std::malloc(sizeof(int64_t) * (found.empty() ? 1 : found.size())));
    if (!a) return genphi_set_error(GENPHI_ERR_ALLOC, "out of memory");
    std::copy(found.begin(), found.end(), a);
    *n_out = static_cast<int64_t>(found.size()); *out = a;
    return GENPHI_OK;
}

// The downward walk of gen.descendant: the children of every individual as one list per parent (start[r] .. start[r + 1],
// positions, in pedigree order; a child whose father is its mother is listed once).
static int child_lists(const char *fn, const IdIndex &pos, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother,
                       std::vector<int64_t> &start, std::vector<int32_t> &child)
{
    std::vector<int32_t> pf(n_ind, -1), pm(n_ind, -1);
    start.assign(n_ind + 1, 0);
    for (int64_t i = 0; i < n_ind; ++i)
        for (int side = 0; side < 2; ++side) {
            const int64_t pid = side ? mother[i] : father[i];
            if (pid == 0 || (side && pid == father[i])) continue;
            const int32_t r = pos.find(pid);
            if (r < 0)
                return genphi_set_error(GENPHI_ERR_UNKNOWN_ID, std::string(fn) + ": KeyError: parent " + std::to_string(pid) + " of " + std::to_string(ind[i]) + " not found");
            (side ? pm : pf)[i] = r;
            start[r + 1]++;
        }
    for (int64_t r = 0; r < n_ind; ++r) start[r + 1] += start[r];
    child.resize(start[n_ind]);
    std::vector<int64_t> fill(start.begin(), start.end() - 1);
    for (int64_t i = 0; i < n_ind; ++i) {
        if (pf[i] >= 0) child[fill[pf[i]]++] = static_cast<int32_t>(i);
        if (pm[i] >= 0) child[fill[pm[i]]++] = static_cast<int32_t>(i);
    }
    return GENPHI_OK;
}

static int ids_out(std::vector<int64_t> &found, int64_t *n_out, int64_t **out)
{
    std::sort(found.begin(), found.end());
    int64_t *a = static_cast<int64_t *>(std::malloc(sizeof(int64_t) * (found.empty() ? 1 : found.size())));
    if (!a) return genphi_set_error(GENPHI_ERR_ALLOC, "out of memory");
    std::copy(found.begin(), found.end(), a);
    *n_out = static_cast<int64_t>(found.size()); *out = a;
    return GENPHI_OK;
}

// gen.descendant (src/identify.jl:203-215): the strict descendants of one ID, or the union over several, ascending.  The
// reference's stack search on positions with one visited flag per individual, as genphi_ancestors.  No order of the pedigree is
// assumed.  *out is allocated by the library (genphi_free).
int genphi_descendants(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_ids, const int64_t *ids,
                       int64_t *n_out, int64_t **out)
{
    if (!n_out || !out || n_ind < 0 || n_ind >= INT32_MAX || n_ids < 0 || (n_ind > 0 && (!ind || !father || !mother)) || (n_ids > 0 && !ids))
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_descendants: bad argument");
    *n_out = 0; *out = nullptr;
    IdIndex pos;
    pos.init(n_ind, ind);
    std::vector<int64_t> stack, found, start;
    std::vector<int32_t> child;
    for (int64_t k = 0; k < n_ids; ++k) {
        const int32_t r = pos.find(ids[k]);
        if (r < 0) return genphi_set_error(GENPHI_ERR_UNKNOWN_ID, "KeyError: individual " + std::to_string(ids[k]) + " not found");
        stack.push_back(r);                          // (an ID is not its own descendant: it is searched, not flagged)
    }
    if (int rc = child_lists("genphi_descendants", pos, n_ind, ind, father, mother, start, child)) return rc;
    std::vector<uint8_t> seen(n_ind, 0);
    while (!stack.empty()) {
        const int64_t i = stack.back();
        stack.pop_back();
        for (int64_t e = start[i]; e < start[i + 1]; ++e) {
            const int32_t c = child[e];
            if (seen[c]) continue;                   // its descendants are on the stack or done
            seen[c] = 1;
            found.push_back(ind[c]);
            stack.push_back(c);
        }
    }
    return ids_out(found, n_out, out);
}

// gen.children (src/identify.jl:77-80): the children of one ID, ascending: one scan of the parent arrays (a single query does not
// pay for the child lists).  *out is allocated by the library (genphi_free).
int genphi_children(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t id, int64_t *n_out, int64_t **out)
{
    if (!n_out || !out || n_ind < 0 || n_ind >= INT32_MAX || (n_ind > 0 && (!ind || !father || !mother)))
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_children: bad argument");
    *n_out = 0; *out = nullptr;
    IdIndex pos;
    pos.init(n_ind, ind);
    if (id == 0 || pos.find(id) < 0) return genphi_set_error(GENPHI_ERR_UNKNOWN_ID, "KeyError: individual " + std::to_string(id) + " not found");
    std::vector<int64_t> found;
    for (int64_t i = 0; i < n_ind; ++i)
        if (father[i] == id || mother[i] == id) found.push_back(ind[i]);
    return ids_out(found, n_out, out);
}

// The last step of _findMRCA (src/identify.jl:97-103): of the common ancestors of a group, keep those that are not an ancestor of
// another common ancestor -- the reference's setdiff(common, ancestor(common)).  Every individual on a path between a common
// ancestor and one of its ancestors is itself common (it is an ancestor of whoever the path leads down to), so a common ancestor
// is "older" exactly when one of its CHILDREN is common: one pass over the parent arrays instead of a search per ancestor.
// `common` must be closed in that sense (it is when it is the full intersection of ancestor sets).  out: room for n_common IDs;
// the kept IDs in the order given.
int genphi_mrca_filter(int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_common,
                       const int64_t *common, int64_t *n_out, int64_t *out)
{
    if (!n_out || n_ind < 0 || n_common < 0 || (n_ind > 0 && (!ind || !father || !mother)) || (n_common > 0 && (!common || !out)))
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_mrca_filter: bad argument");
    *n_out = 0;
    IdIndex pos;
    pos.init(n_ind, ind);
    std::vector<uint8_t> older(n_ind, 0);
    for (int64_t k = 0; k < n_common; ++k) {
        const int32_t i = pos.find(common[k]);
        if (i < 0) return genphi_set_error(GENPHI_ERR_UNKNOWN_ID, "KeyError: individual " + std::to_string(common[k]) + " not found");
        for (int side = 0; side < 2; ++side) {
            const int64_t pid = side ? mother[i] : father[i];
            const int32_t r = pid == 0 ? -1 : pos.find(pid);
            if (r >= 0) older[r] = 1;                        // a parent of a common ancestor
        }
    }
    int64_t m = 0;
    for (int64_t k = 0; k < n_common; ++k)
        if (!older[pos.find(common[k])]) out[m++] = common[k];
    *n_out = m;
    return GENPHI_OK;
}

}  // extern "C"
