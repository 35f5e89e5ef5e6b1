// ancestor_sweep.cpp -- host schedule of the ancestor x proband sweeps (see ancestor_sweep.h).
#include "ancestor_sweep.h"

#include <algorithm>

#include "../../include/genphi.h"
#include "planner.h"

namespace genphi {

int plan_sweep(SweepSchedule &h, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
               const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, const SweepOptions &sopt, std::string &err)
{
    h = SweepSchedule();
    Ranks ranks;
    std::vector<int64_t> known_pro;
    if (sopt.drop_unknown_pro) {
        ranks.init(n_ind, ind);
        for (int64_t k = 0; k < n_pro; ++k)
            if (ranks.find(pro_ids[k]) >= 0) known_pro.push_back(pro_ids[k]);
        n_pro = static_cast<int64_t>(known_pro.size());
        pro_ids = known_pro.data();
    }
    PlanOptions opt;
    opt.indices_only = true;
    Plan plan;
    // (validates the pedigree -- order, duplicates -- and the proband IDs; the planner keeps first occurrences)
    int rc = build_plan(n_ind, ind, father, mother, n_pro, pro_ids, opt, plan, err);
    if (rc) return rc;
    if (!sopt.drop_unknown_pro) ranks.init(n_ind, ind);
    std::vector<int32_t> anc_rank(n_anc);
    for (int64_t j = 0; j < n_anc; ++j) {
        anc_rank[j] = ranks.find(anc_ids[j]);
        if (anc_rank[j] < 0) { err = "KeyError: ancestor " + std::to_string(anc_ids[j]) + " not found"; return GENPHI_ERR_UNKNOWN_ID; }
    }
    h.n_pro = n_pro; h.n_anc = n_anc;
    const int L = plan.n_levels;
    h.n_steps = std::max(L - 1, 0);
    if (sopt.emit == Emit::None) {
        std::vector<char> is_pro(n_ind, 0);
        for (int64_t k = 0; k < n_pro; ++k) is_pro[ranks.find(pro_ids[k])] = 1;
        h.anc_is_pro.resize(n_anc);
        for (int64_t j = 0; j < n_anc; ++j) h.anc_is_pro[j] = is_pro[anc_rank[j]];
    }
    if (n_pro == 0 || (n_anc == 0 && !sopt.every_member) || L == 0) return GENPHI_OK;

    // parents as ranks (the planner checked that they exist and come first), leaves, relevance
    std::vector<int32_t> fa(n_ind, -1), mo(n_ind, -1);
    std::vector<char> has_child(n_ind, 0), rel(n_ind, 0);
    for (int64_t i = 0; i < n_ind; ++i) {
        if (father[i] != 0) { fa[i] = ranks.find(father[i]); has_child[fa[i]] = 1; }
        if (mother[i] != 0) { mo[i] = ranks.find(mother[i]); has_child[mo[i]] = 1; }
    }
    // one-hot columns of each ancestor rank: CSR over the ranks that are requested (columns ascending)
    std::vector<int32_t> oh_start(n_ind + 1, 0);
    for (int64_t j = 0; j < n_anc; ++j) oh_start[anc_rank[j] + 1]++;
    for (int64_t i = 0; i < n_ind; ++i) oh_start[i + 1] += oh_start[i];
    std::vector<int32_t> oh_of(n_anc);
    {
        std::vector<int32_t> fill(oh_start.begin(), oh_start.end() - 1);
        for (int64_t j = 0; j < n_anc; ++j) oh_of[fill[anc_rank[j]]++] = static_cast<int32_t>(j);
    }
    for (int64_t i = 0; i < n_ind; ++i)      // rank order: parents first
        rel[i] = sopt.every_member || oh_start[i + 1] > oh_start[i] || (fa[i] >= 0 && rel[fa[i]]) || (mo[i] >= 0 && rel[mo[i]]);
    if (sopt.every_member) {
        // generations = 1 + the longest ascent of a listed proband, from the depths of the ranks (founders 1)
        std::vector<int32_t> depth(n_ind, 1);
        for (int64_t i = 0; i < n_ind; ++i)
            depth[i] = 1 + std::max(fa[i] >= 0 ? depth[fa[i]] : 0, mo[i] >= 0 ? depth[mo[i]] : 0);
        for (int64_t k = 0; k < n_pro; ++k) h.n_generations = std::max(h.n_generations, depth[ranks.find(pro_ids[k])]);
    }

    // members of cut 0 (founders) by position, from the sources of cut 1 (every member of cut 0 is one of them)
    std::vector<int32_t> cut0(plan.cut_sizes[0], -1);
    if (L == 1) {
        for (int64_t k = 0; k < plan.cut_sizes[0]; ++k) cut0[k] = plan.final_members[k];
    } else {
        const LevelStep &st = plan.steps[0];
        const int32_t none = static_cast<int32_t>(st.n_prev);
        for (int64_t k = 0; k < st.n; ++k) {
            const int32_t o = st.ord[k];
            if (o >= 0) { cut0[st.srcA[k]] = o; continue; }
            const int32_t x = o & 0x7fffffff;
            if (st.srcA[k] != none) cut0[st.srcA[k]] = fa[x] >= 0 ? fa[x] : mo[x];
            if (st.srcB[k] != none) cut0[st.srcB[k]] = mo[x];
        }
    }
    // result rows of each distinct proband: CSR over the ranks, rows ascending.  LeafFirst: the first occurrence in pro_ids only.
    std::vector<int32_t> row_start(n_ind + 1, 0), row_of;
    const bool emits = sopt.emit != Emit::None;
    if (emits) {
        std::vector<int32_t> pro_rank(n_pro);
        for (int64_t k = 0; k < n_pro; ++k) pro_rank[k] = ranks.find(pro_ids[k]);
        std::vector<char> seen(n_ind, 0);
        std::vector<char> listed(n_pro, 0);
        for (int64_t k = 0; k < n_pro; ++k) {
            listed[k] = sopt.emit == Emit::EveryProband || !seen[pro_rank[k]];
            seen[pro_rank[k]] = 1;
            if (listed[k]) row_start[pro_rank[k] + 1]++;
        }
        for (int64_t i = 0; i < n_ind; ++i) row_start[i + 1] += row_start[i];
        row_of.resize(row_start[n_ind]);
        std::vector<int32_t> fill(row_start.begin(), row_start.end() - 1);
        for (int64_t k = 0; k < n_pro; ++k)
            if (listed[k]) row_of[fill[pro_rank[k]]++] = static_cast<int32_t>(k);
    }

    auto add_item = [&](int32_t dst, int32_t A, int32_t B, int32_t x, bool onehot) {
        h.items.push_back(SweepItem{dst, A, B, static_cast<int32_t>(h.oh_cols.size())});
        if (onehot)
            for (int32_t q = oh_start[x]; q < oh_start[x + 1]; ++q) {
                h.oh_cols.push_back(oh_of[q]);
                if (sopt.first_onehot_only) break;
            }
        h.list_srcs.back() += (A >= 0) + (B >= 0);
    };
    // one result row per listed occurrence of proband x
    auto emit_rows = [&](int32_t A, int32_t B, int32_t x, bool onehot) {
        for (int32_t q = row_start[x]; q < row_start[x + 1]; ++q) add_item(row_of[q], A, B, x, onehot);
    };
    auto open_list = [&](bool to_result) {
        h.list_begin.push_back(static_cast<int64_t>(h.items.size()));
        h.list_to_result.push_back(to_result);
        h.list_srcs.push_back(0.0);
    };
    auto close_list = [&]() { h.items.push_back(SweepItem{-1, -1, -1, static_cast<int32_t>(h.oh_cols.size())}); };
    auto emitted = [&](int32_t x) { return rel[x] && (sopt.emit == Emit::EveryProband || !has_child[x]); };

    // slots: a free list; slot_of_prev = slots of the members of the current source cut by position (-1 = zero row)
    std::vector<int32_t> free_slots;
    int32_t n_slots = 0;
    auto take = [&]() -> int32_t {
        if (!free_slots.empty()) { const int32_t s = free_slots.back(); free_slots.pop_back(); return s; }
        return n_slots++;
    };
    std::vector<int32_t> slot_prev(plan.cut_sizes[0], -1);
    open_list(L == 1 && emits);
    for (int64_t k = 0; k < plan.cut_sizes[0]; ++k) {
        const int32_t x = cut0[k];
        if (L == 1 && emits) {
            if (emitted(x)) emit_rows(-1, -1, x, true);
        } else if (rel[x]) {
            slot_prev[k] = take();
            add_item(slot_prev[k], -1, -1, x, true);
        }
    }
    close_list();
    std::vector<int32_t> rows;
    for (int s = 0; s + 1 < L; ++s) {
        const LevelStep &st = plan.steps[s];
        const bool last = emits && s + 2 == L;
        const int32_t none = static_cast<int32_t>(st.n_prev);
        std::vector<int32_t> slot_cur(st.n, -1);
        std::vector<char> kept(st.n_prev, 0);
        rows.clear();
        for (int64_t k = 0; k < st.n; ++k) {
            const int32_t o = st.ord[k];
            if (o >= 0) { slot_cur[k] = slot_prev[st.srcA[k]]; kept[st.srcA[k]] = 1; continue; }   // dragged: same slot
            const int32_t x = o & 0x7fffffff;
            if (last ? emitted(x) : rel[x]) rows.push_back(static_cast<int32_t>(k));
        }
        reuse_order(st, rows);                                // siblings adjacent: the shared source row is served by L2
        open_list(last);
        for (int32_t k : rows) {
            const int32_t x = st.ord[k] & 0x7fffffff;
            const int32_t A = st.srcA[k] == none ? -1 : slot_prev[st.srcA[k]];
            const int32_t B = st.srcB[k] == none ? -1 : slot_prev[st.srcB[k]];
            if (last) { emit_rows(A, B, x, true); continue; }
            slot_cur[k] = take();
            add_item(slot_cur[k], A, B, x, true);
        }
        if (last && sopt.emit == Emit::EveryProband)
            // probands dragged into the last cut: their rows were finished by an earlier step and wait in their slots
            for (int64_t k = 0; k < st.n; ++k)
                if (st.ord[k] >= 0 && slot_cur[k] >= 0) emit_rows(slot_cur[k], sopt.mark_copies ? -2 : -1, st.ord[k], false);
        close_list();
        // members of the source cut that leave with this step: their slots serve the steps after it
        for (int64_t q = 0; q < st.n_prev; ++q)
            if (!kept[q] && slot_prev[q] >= 0) free_slots.push_back(slot_prev[q]);
        slot_prev.swap(slot_cur);
    }
    h.peak_slots = n_slots;                                   // (slots are taken from the free list first: the most ever live at once)
    h.list_begin.push_back(static_cast<int64_t>(h.items.size()));
    if (!emits)
        for (int32_t s : slot_prev)
            if (s >= 0) h.pro_slots.push_back(s);
    return GENPHI_OK;
}

}  // namespace genphi
