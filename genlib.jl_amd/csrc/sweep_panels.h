// sweep_panels.h -- column panels of the ancestor sweeps (gen.gc, gen.occ, gen.rec, gen.meioses): how wide a panel is, its row
// pitch, how many panels there are and how many one launch covers; no HIP here (tests/sweep_panels_check.cpp runs it on the CPU).
//
// The columns of a sweep are independent: it runs over panels of C columns, each with its own peak_slots slot rows.  Default
// panels are as wide as keeps the slot rows of one panel within about 150 MiB (kPanelSlotBytes), so that a panel's live rows
// stay in the 256 MiB Infinity Cache between the step that writes them and the steps that read them; one panel per launch, panels
// one after the other.  Measured against one panel of every column: cfg3 x 6,633 founders 1.53 vs 1.96 ms, cfg4 x
// 50,366 founders 122 vs 140 ms.  A sweep's *_PANEL hook sets C instead, its *_PANELS_PER_LAUNCH hook the panels of a launch.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace genphi {

constexpr double kPanelSlotBytes = 150.0 * 1048576.0;

// What a sweep's rows are made of.  Rows are moved 16 bytes at a time: the pitch is a multiple of vec_elems elements.
struct PanelRule {
    int64_t elem_bytes;          // bytes of a row element
    int64_t cols_per_elem;       // columns an element holds: 1, or 64 for bit rows
    int64_t vec_elems;           // elements per 16 bytes
    int64_t min_cols;            // the default C is at least this (narrower rows are too short for the 16-byte row gather)
    int64_t default_multiple;    // ... and a multiple of this
    int64_t halve_multiple;      // where a default panel does not fit, C is halved: to max(halve_floor, a multiple of this), or --
    int64_t halve_floor;         // halve_multiple 0 -- to (C + 1) / 2; until it fits or C <= halve_floor
    int64_t elems(int64_t cols) const { return (cols + cols_per_elem - 1) / cols_per_elem; }
    int64_t pitch(int64_t cols) const { return (elems(cols) + vec_elems - 1) / vec_elems * vec_elems; }
};

struct PanelLayout {
    int64_t slots = 0;           // slot rows of a panel: max(peak_slots, 1)
    int64_t C = 0;               // columns of a panel (the last one may have fewer)
    int32_t Cp = 0;              // row pitch in elements
    int64_t n_panels = 0;
    int64_t per_launch = 0;      // panels a launch covers (grid dimension y)
    long long stride = 0;        // elements of one panel: slots * Cp
    size_t slot_bytes = 0;       // per_launch panels
    // bytes of one row over panels [p0, p0 + n) of n_cols columns (algorithmic bytes)
    double row_bytes(const PanelRule &r, int64_t n_cols, int64_t p0, int64_t n) const
    {
        double b = 0.0;
        for (int64_t p = p0; p < p0 + n; ++p) b += static_cast<double>(r.elem_bytes * r.elems(std::min<int64_t>(C, n_cols - p * C)));
        return b;
    }
};

// panel_env / group_env: the sweep's hooks (0 = the default rule); slot_room: the device bytes the slot rows may take.
// Nonzero: not even the narrowest panel fits (out.slots and out.C say what was tried).
static inline int plan_panels(PanelLayout &out, const PanelRule &rule, int64_t peak_slots, int64_t n_cols, int32_t panel_env, int32_t group_env,
                              double slot_room)
{
    const int64_t S = std::max<int64_t>(peak_slots, 1);
    auto panel_bytes = [&](int64_t c) { return static_cast<double>(rule.elem_bytes) * static_cast<double>(S) * static_cast<double>(rule.pitch(c)); };
    int64_t C = panel_env;
    if (panel_env <= 0) {
        const double fit = kPanelSlotBytes * static_cast<double>(rule.cols_per_elem) / static_cast<double>(rule.elem_bytes * S);
        C = std::max(rule.min_cols, static_cast<int64_t>(fit) / rule.default_multiple * rule.default_multiple);
    }
    C = std::min(C, std::max<int64_t>(n_cols, 1));
    if (panel_env <= 0)
        while (C > rule.halve_floor && panel_bytes(C) > slot_room)          // (more slot rows than the device holds at that width)
            C = rule.halve_multiple ? std::max(rule.halve_floor, C / 2 / rule.halve_multiple * rule.halve_multiple) : (C + 1) / 2;
    out.slots = S;
    out.C = C;
    if (panel_bytes(C) > slot_room) return 1;
    out.n_panels = (n_cols + C - 1) / C;
    // panels per launch: one by default; with the panel hook as many as the memory holds, unless the per-launch hook says otherwise
    const int64_t held = static_cast<int64_t>(slot_room / panel_bytes(C));
    int64_t G = 1;
    if (panel_env > 0) G = std::max<int64_t>(1, std::min(out.n_panels, held));
    if (group_env > 0) G = group_env;
    out.per_launch = std::max<int64_t>(1, std::min<int64_t>({G, out.n_panels, 65535, held}));
    out.Cp = static_cast<int32_t>(rule.pitch(C));
    out.stride = static_cast<long long>(S) * out.Cp;
    out.slot_bytes = static_cast<size_t>(out.per_launch) * static_cast<size_t>(out.stride) * static_cast<size_t>(rule.elem_bytes);
    return 0;
}

}  // namespace genphi
