// implex.cpp -- host plan of gen.implex (see implex.h): the union frontier per generation and its child lists, O(sum of |U_g|).
#include "implex.h"

#include <algorithm>

#include "../../include/genphi.h"
#include "pedigree_index.h"

namespace genphi {

int plan_implex(ImplexPlan &h, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
                const int64_t *pro_ids, int32_t max_generations, std::string &err)
{
    h = ImplexPlan();
    PedigreeIndex px;
    if (const int rc = index_pedigree(px, n_ind, ind, father, mother, err)) return rc;
    const std::vector<int32_t> &fa = px.fa, &mo = px.mo;
    std::vector<int32_t> depth(n_ind, 1);
    for (int64_t i = 0; i < n_ind; ++i) depth[i] = 1 + std::max(fa[i] >= 0 ? depth[fa[i]] : 0, mo[i] >= 0 ? depth[mo[i]] : 0);
    // ---- U_0: the distinct probands, with the columns of their listed occurrences ----
    std::vector<int32_t> stamp(n_ind, -1), pos(n_ind, -1), uid(n_ind, -1);
    std::vector<int32_t> cur, nxt, pro_rank;
    if (const int rc = find_probands(pro_rank, px.ranks, n_pro, pro_ids, err)) return rc;
    int32_t G = 0;
    for (int32_t r : pro_rank) {
        G = std::max(G, depth[r]);
        if (stamp[r] != 0) { stamp[r] = 0; pos[r] = static_cast<int32_t>(cur.size()); cur.push_back(r); }
    }
    h.n_pro = n_pro;
    h.G = G;
    if (G - 1 > max_generations) {
        err = "gen.implex: " + std::to_string(G - 1) + " generations above the probands; the 2^g of the percentages holds at most " +
              std::to_string(max_generations);
        return GENPHI_ERR_ARG;
    }
    if (n_pro == 0) return GENPHI_OK;
    h.occ_start.assign(cur.size() + 1, 0);
    for (int64_t k = 0; k < n_pro; ++k) h.occ_start[pos[pro_rank[k]] + 1]++;
    for (size_t r = 0; r < cur.size(); ++r) h.occ_start[r + 1] += h.occ_start[r];
    h.occ_cols.resize(n_pro);
    {
        std::vector<int32_t> fill(h.occ_start.begin(), h.occ_start.end() - 1);
        for (int64_t k = 0; k < n_pro; ++k) h.occ_cols[fill[pos[pro_rank[k]]]++] = static_cast<int32_t>(k);
    }
    auto close_generation = [&](const std::vector<int32_t> &members) {
        h.rows.push_back(static_cast<int64_t>(members.size()));
        for (int32_t x : members) {
            if (uid[x] < 0) { uid[x] = static_cast<int32_t>(h.n_union++); h.seen_row.push_back(~uid[x]); }
            else h.seen_row.push_back(uid[x]);
        }
        h.row_begin.push_back(static_cast<int64_t>(h.seen_row.size()));
        h.start_begin.push_back(static_cast<int64_t>(h.edge_start.size()));
        h.child_begin.push_back(static_cast<int64_t>(h.child.size()));
    };
    h.row_begin.push_back(0);
    h.start_begin.push_back(0);
    h.child_begin.push_back(0);
    close_generation(cur);
    // ---- U_g from U_{g-1}: the distinct known parents, and per parent the positions of its children ----
    std::vector<int32_t> cnt;
    for (int32_t g = 1; g < G; ++g) {
        nxt.clear();
        cnt.clear();
        auto meet = [&](int32_t p) {
            if (stamp[p] != g) { stamp[p] = g; pos[p] = static_cast<int32_t>(nxt.size()); nxt.push_back(p); cnt.push_back(0); }
            cnt[pos[p]]++;
        };
        for (int32_t x : cur) {
            if (fa[x] >= 0) meet(fa[x]);
            if (mo[x] >= 0 && mo[x] != fa[x]) meet(mo[x]);
        }
        const size_t s0 = h.edge_start.size(), c0 = h.child.size();
        h.edge_start.resize(s0 + nxt.size() + 1);
        int32_t *start = h.edge_start.data() + s0;
        start[0] = 0;
        for (size_t r = 0; r < nxt.size(); ++r) start[r + 1] = start[r] + cnt[r];
        h.child.resize(c0 + static_cast<size_t>(start[nxt.size()]));
        int32_t *child = h.child.data() + c0;
        std::fill(cnt.begin(), cnt.end(), 0);
        for (size_t q = 0; q < cur.size(); ++q) {
            const int32_t x = cur[q];
            if (fa[x] >= 0) { const int32_t r = pos[fa[x]]; child[start[r] + cnt[r]++] = static_cast<int32_t>(q); }
            if (mo[x] >= 0 && mo[x] != fa[x]) { const int32_t r = pos[mo[x]]; child[start[r] + cnt[r]++] = static_cast<int32_t>(q); }
        }
        cur.swap(nxt);
        close_generation(cur);
    }
    for (int64_t r : h.rows) { h.peak_rows = std::max(h.peak_rows, r); h.sum_rows += r; }
    h.sum_edges = static_cast<int64_t>(h.child.size());
    return GENPHI_OK;
}

}  // namespace genphi
