// device_sizes.h -- what a plan's Float32 sweep needs on the device, as a pure function of the Plan (host only, no HIP).
//
// The upload, the allocation of the level buffers, the per-call buffers and genphi_plan_device_bytes_needed all read these figures: the
// estimate that decides what fits on a GPU (bench.py, distributed.py) cannot drift from what is allocated.  (The index blob is sized by
// the code that fills it -- BlobPacker in genphi_hip.hip --, which needs the walk lists; the estimate keeps a formula for that one.)
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "planner.h"

namespace genphi {

// level matrices carry a zeroed tail so that the SPLIT kernel's unconditional staging loads
// (STG * 1024 float4 per row, <= 160 KB) may run past the last row
constexpr size_t kTailPadFloats = 64 * 1024;

struct DeviceSizes {
    // which of the two level buffers holds cut c: alternating, except that a WIDE step that stays in place (LevelStep::stay)
    // writes into its source's buffer.  buf_of[0]: with in-place steps (the product sweep), buf_of[1]: plain alternation (the
    // per-entry kernel = 1 sweep, which knows no slots).  cert_cut[c]: the cut whose certificate words cut c shares in the
    // product sweep (the entry cut of its in-place run; c itself otherwise); L + 1 entries, the last one L.
    std::vector<int> buf_of[2], cert_cut;
    // exactness certificates, one word per row of every level matrix: words [cert_off[c], cert_off[c + 1]) belong to cut c (incl. its
    // "none" row; a cut stored by slot has one word per slot).  L + 1 entries: cert_off[L] is the total.
    std::vector<size_t> cert_off;
    std::vector<size_t> cut_floats;            // per intermediate cut c < L - 1: its matrix (rows + the "none" row) + the tail pad
    size_t psi_p_floats = 0, psi_p_rows = 0;   // WIDE: the compacted parent matrix (0: none), its rows incl. "none"
    size_t nn_pad = 0, nn_tmp_floats = 0;      // in-place WIDE steps: the widest new x new block is nn_pad x nn_pad (+ the tail pad)
    size_t final_tmp_floats = 0;               // the whole last level in storage order, for the sweeps that deliver it by a permutation pass

    // floats each level buffer needs when cuts first_cut .. L-2 exist as matrices: a buffer serves the sweep with in-place steps AND the
    // plain alternation of the per-entry sweep
    void level_buffers(int first_cut, size_t need[2]) const
    {
        need[0] = need[1] = 0;
        for (size_t c = static_cast<size_t>(std::max(first_cut, 0)); c < cut_floats.size(); ++c)
            for (int v = 0; v < 2; ++v) need[buf_of[v][c]] = std::max(need[buf_of[v][c]], cut_floats[c]);
    }
};

// rows [0, n_rows) of the result at the pitch of the last cut (the run's pitch when the proband cut stays in place)
inline size_t result_floats(const Plan &pl, int64_t n_rows) { return pl.n_levels ? static_cast<size_t>(n_rows * pl.ld[pl.n_levels - 1]) : 0; }

inline DeviceSizes device_sizes(const Plan &pl)
{
    DeviceSizes z;
    const int L = pl.n_levels;
    z.cert_off.assign(L + 1, 0);
    z.cert_cut.assign(L + 1, 0);
    z.buf_of[0].assign(L, 0); z.buf_of[1].assign(L, 0);
    size_t w = 0;
    for (int c = 0; c < L; ++c) {
        z.cert_off[c] = w;
        // a cut stored by slot (the source of a step with src_slots: the cuts of an in-place run of WIDE steps): P slots + the "none" row P,
        // pitch P = ld[c]
        const bool by_slot = c < static_cast<int>(pl.steps.size()) && pl.steps[c].src_slots;
        const size_t rows = (by_slot ? static_cast<size_t>(pl.steps[c].P) : static_cast<size_t>(pl.cut_sizes[c])) + 1;
        w += rows;
        if (c + 1 < L) z.cut_floats.push_back(rows * static_cast<size_t>(pl.ld[c]) + kTailPadFloats);
        const bool stays = c >= 1 && pl.steps[c - 1].stay;
        z.cert_cut[c] = stays ? z.cert_cut[c - 1] : c;
        if (c >= 1) { z.buf_of[0][c] = stays ? z.buf_of[0][c - 1] : 1 - z.buf_of[0][c - 1]; z.buf_of[1][c] = c & 1; }
    }
    z.cert_cut[L] = L;
    z.cert_off[L] = w;
    for (const LevelStep &st : pl.steps) {
        if (st.mode == kModeWide && !st.nn.empty()) {          // the new x new sub-step runs on Psi[parents][parents]
            z.psi_p_floats = std::max(z.psi_p_floats, static_cast<size_t>((st.nn[0].n_prev + 1) * st.nn[0].ld_prev) + kTailPadFloats);
            z.psi_p_rows = std::max(z.psi_p_rows, static_cast<size_t>(st.nn[0].n_prev) + 1);
        }
        if (st.stay) z.nn_pad = std::max(z.nn_pad, static_cast<size_t>(st.npad));
    }
    if (z.nn_pad) z.nn_tmp_floats = z.nn_pad * z.nn_pad + kTailPadFloats;
    if (L) z.final_tmp_floats = static_cast<size_t>((pl.n_pro + 1) * pl.ld[L - 1]) + kTailPadFloats;
    return z;
}

}  // namespace genphi
