// sweep_panels_check.cpp -- plan_panels (csrc/sweep_panels.h, no HIP) against
//   (a) the panel arithmetic as gen.gc, gen.occ / gen.rec and gen.meioses each wrote it out before they shared plan_panels, restated
//       here one sweep at a time (never by calling plan_panels), over a grid of slots x columns x hooks x device room;
//   (b) layouts derived by hand;
//   (c) what every layout has to satisfy.
// Prints one summary line; a violation is reported on stderr and counted.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../genlib.jl_amd/csrc/sweep_panels.h"

namespace {

using genphi::PanelLayout;
using genphi::PanelRule;

constexpr double kSlotBytes = 150.0 * 1048576.0;      // 157,286,400

struct Ref {
    bool fits = false;
    int64_t C = 0, Cp = 0, n_panels = 0, G = 0;
    long long stride = 0;
    size_t slot_bytes = 0;
};

// gen.gc: Float64 rows, the pitch is C up to even
Ref ref_gc(int64_t peak_slots, int64_t n_anc, int32_t panel_env, int32_t group_env, double slot_room)
{
    Ref r;
    const int64_t S = std::max<int64_t>(peak_slots, 1);
    int64_t C = panel_env > 0 ? panel_env : std::max<int64_t>(64, static_cast<int64_t>(kSlotBytes / (8.0 * S)));
    C = std::min(C, std::max<int64_t>(n_anc, 1));
    auto panel_bytes = [&](int64_t c) { return 8.0 * static_cast<double>(S) * static_cast<double>((c + 1) & ~int64_t(1)); };
    if (panel_env <= 0)
        while (C > 1 && panel_bytes(C) > slot_room) C = (C + 1) / 2;
    r.C = C;
    if (panel_bytes(C) > slot_room) return r;
    r.fits = true;
    r.n_panels = n_anc > 0 ? (n_anc + C - 1) / C : 0;
    int64_t G = 1;
    if (panel_env > 0) G = std::max<int64_t>(1, std::min<int64_t>(r.n_panels, static_cast<int64_t>(slot_room / panel_bytes(C))));
    if (group_env > 0) G = group_env;
    G = std::max<int64_t>(1, std::min<int64_t>({G, r.n_panels, 65535, static_cast<int64_t>(slot_room / panel_bytes(C))}));
    r.G = G;
    r.Cp = (C + 1) & ~int64_t(1);
    r.stride = static_cast<long long>(S) * r.Cp;
    r.slot_bytes = static_cast<size_t>(G) * static_cast<size_t>(r.stride) * sizeof(double);
    return r;
}

// gen.occ (rows of 4 or 8 bytes) and gen.rec (bits: 64 columns per 8-byte word)
Ref ref_occ(bool bits, int row_bits, int64_t peak_slots, int64_t n_anc, int32_t panel_env, int32_t group_env, double slot_room)
{
    Ref r;
    const int64_t esize = bits ? 8 : row_bits / 8;
    const int64_t V = 16 / esize;
    auto elems = [&](int64_t c) { return bits ? (c + 63) / 64 : c; };
    auto pitch = [&](int64_t c) { return (elems(c) + V - 1) / V * V; };
    const int64_t S = std::max<int64_t>(peak_slots, 1);
    int64_t C;
    if (panel_env > 0) C = panel_env;
    else if (bits) C = std::max<int64_t>(4096, static_cast<int64_t>(kSlotBytes * 8.0 / static_cast<double>(S)) / 128 * 128);
    else C = std::max<int64_t>(64, static_cast<int64_t>(kSlotBytes / static_cast<double>(esize * S)));
    C = std::min(C, std::max<int64_t>(n_anc, 1));
    auto panel_bytes = [&](int64_t c) { return static_cast<double>(esize) * static_cast<double>(S) * static_cast<double>(pitch(c)); };
    if (panel_env <= 0)
        while (C > 1 && panel_bytes(C) > slot_room) C = bits ? std::max<int64_t>(1, C / 2 / 64 * 64) : (C + 1) / 2;
    r.C = C;
    if (panel_bytes(C) > slot_room) return r;
    r.fits = true;
    r.n_panels = (n_anc + C - 1) / C;
    int64_t G = 1;
    if (panel_env > 0) G = std::max<int64_t>(1, std::min<int64_t>(r.n_panels, static_cast<int64_t>(slot_room / panel_bytes(C))));
    if (group_env > 0) G = group_env;
    G = std::max<int64_t>(1, std::min<int64_t>({G, r.n_panels, 65535, static_cast<int64_t>(slot_room / panel_bytes(C))}));
    r.G = G;
    r.Cp = pitch(C);
    r.stride = static_cast<long long>(S) * r.Cp;
    r.slot_bytes = static_cast<size_t>(G) * static_cast<size_t>(r.stride) * static_cast<size_t>(esize);
    return r;
}

// gen.meioses: 16-bit rows, 8 columns per 16 bytes
Ref ref_dist(int64_t peak_slots, int64_t n_anc, int32_t panel_env, int32_t group_env, double slot_room)
{
    Ref r;
    constexpr int64_t kRowBytes = 2, kVec = 8;
    auto pitch = [&](int64_t c) { return (c + kVec - 1) / kVec * kVec; };
    const int64_t S = std::max<int64_t>(peak_slots, 1);
    int64_t C;
    if (panel_env > 0) C = panel_env;
    else C = std::max<int64_t>(64, static_cast<int64_t>(kSlotBytes / static_cast<double>(kRowBytes * S)) / kVec * kVec);
    C = std::min(C, std::max<int64_t>(n_anc, 1));
    auto panel_bytes = [&](int64_t c) { return static_cast<double>(kRowBytes) * static_cast<double>(S) * static_cast<double>(pitch(c)); };
    if (panel_env <= 0)
        while (C > kVec && panel_bytes(C) > slot_room) C = std::max<int64_t>(kVec, C / 2 / kVec * kVec);
    r.C = C;
    if (panel_bytes(C) > slot_room) return r;
    r.fits = true;
    r.n_panels = (n_anc + C - 1) / C;
    int64_t G = 1;
    if (panel_env > 0) G = std::max<int64_t>(1, std::min<int64_t>(r.n_panels, static_cast<int64_t>(slot_room / panel_bytes(C))));
    if (group_env > 0) G = group_env;
    G = std::max<int64_t>(1, std::min<int64_t>({G, r.n_panels, 65535, static_cast<int64_t>(slot_room / panel_bytes(C))}));
    r.G = G;
    r.Cp = pitch(C);
    r.stride = static_cast<long long>(S) * r.Cp;
    r.slot_bytes = static_cast<size_t>(G) * static_cast<size_t>(r.stride) * static_cast<size_t>(kRowBytes);
    return r;
}

// the rules as the sweeps state them (gc.hip, occ.hip, dist.hip)
constexpr PanelRule kGc = {8, 1, 2, 64, 1, 0, 1}, kOcc32 = {4, 1, 4, 64, 1, 0, 1}, kOcc64 = {8, 1, 2, 64, 1, 0, 1}, kRec = {8, 64, 2, 4096, 128, 64, 1},
                    kDist = {2, 1, 8, 64, 8, 8, 8};
enum Sweep { Gc, Occ32, Occ64, Rec, Dist, kSweeps };
const char *const kNames[kSweeps] = {"gc", "occ32", "occ64", "rec", "meioses"};
const PanelRule *const kRules[kSweeps] = {&kGc, &kOcc32, &kOcc64, &kRec, &kDist};

Ref reference(int sweep, int64_t S, int64_t n, int32_t panel, int32_t group, double room)
{
    switch (sweep) {
    case Gc: return ref_gc(S, n, panel, group, room);
    case Occ32: return ref_occ(false, 32, S, n, panel, group, room);
    case Occ64: return ref_occ(false, 64, S, n, panel, group, room);
    case Rec: return ref_occ(true, 64, S, n, panel, group, room);
    default: return ref_dist(S, n, panel, group, room);
    }
}

long long violations = 0;

#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            ++violations;                                     \
            std::fprintf(stderr, "VIOLATION: " __VA_ARGS__);  \
            std::fprintf(stderr, " (%s)\n", #cond);           \
        }                                                     \
    } while (0)

struct Pin {
    int sweep;
    int64_t S, n;
    int32_t panel, group;
    double room;
    int64_t C, Cp, n_panels, G;      // -1: not pinned
};

}  // namespace

int main()
{
    const int64_t slots[] = {1, 2, 63, 1000, 1000000, 30000000};
    const int64_t cols[] = {1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 100000};
    const int32_t panels[] = {0, 1, 3, 8, 64, 65, 100, 104};
    const int32_t groups[] = {0, 1, 7};
    const double rooms[] = {4096.0, 1048576.0, 50e6, 1e12};
    long long cases = 0, fit = 0, no_fit = 0;
    for (int sw = 0; sw < kSweeps; ++sw)
        for (int64_t S : slots)
            for (int64_t n : cols)
                for (int32_t panel : panels)
                    for (int32_t group : groups)
                        for (double room : rooms) {
                            const PanelRule &rule = *kRules[sw];
                            const Ref ref = reference(sw, S, n, panel, group, room);
                            PanelLayout L;
                            const int rc = genphi::plan_panels(L, rule, S, n, panel, group, room);
                            ++cases;
#define WHERE "%s S %lld n %lld panel %d group %d room %.0f", kNames[sw], (long long)S, (long long)n, panel, group, room
                            CHECK((rc == 0) == ref.fits, WHERE);
                            CHECK(L.C == ref.C && L.slots == S, WHERE);
                            if (rc || !ref.fits) { ++no_fit; continue; }
                            ++fit;
                            CHECK(L.Cp == ref.Cp && L.n_panels == ref.n_panels && L.per_launch == ref.G, WHERE);
                            CHECK(L.stride == ref.stride && L.slot_bytes == ref.slot_bytes, WHERE);
                            // (c)
                            const int64_t el = (L.C + rule.cols_per_elem - 1) / rule.cols_per_elem;
                            CHECK(L.Cp >= el && L.Cp % rule.vec_elems == 0, WHERE);
                            CHECK(L.per_launch >= 1 && L.per_launch <= std::min<int64_t>(L.n_panels, 65535), WHERE);
                            const double panel_bytes = static_cast<double>(rule.elem_bytes) * static_cast<double>(S) * static_cast<double>(L.Cp);
                            CHECK(static_cast<double>(L.per_launch) * panel_bytes <= room, WHERE);
                            CHECK(static_cast<double>(L.slot_bytes) == static_cast<double>(L.per_launch) * panel_bytes, WHERE);
                            CHECK(L.n_panels * L.C >= n && n > (L.n_panels - 1) * L.C, WHERE);
                            // the bytes of a row over every panel: the bytes of its n columns' elements, panel by panel
                            double want = 0.0;
                            for (int64_t p = 0; p < L.n_panels; ++p)
                                want += static_cast<double>(rule.elem_bytes * ((std::min(L.C, n - p * L.C) + rule.cols_per_elem - 1) / rule.cols_per_elem));
                            CHECK(L.row_bytes(rule, n, 0, L.n_panels) == want, WHERE);
                        }
    // (b) by hand, with 150 MiB = 157,286,400 bytes
    const Pin pins[] = {
        {Gc, 1000, 100000, 0, 0, 1e12, 19660, 19660, 6, 1},      // 157,286,400 / 8,000 = 19,660.8; 5 x 19,660 < 100,000
        {Gc, 1000, 100000, 0, 0, 50e6, 4915, 4916, -1, 1},       // 19,660 -> 9,830 (78.6 MB) -> 4,915 at a pitch of 4,916 (39.3 MB)
        {Gc, 1, 10, 0, 0, 1e12, 10, 10, 1, -1},
        {Occ32, 1000, 100000, 0, 0, 1e12, 39321, 39324, 3, -1},  // 157,286,400 / 4,000 = 39,321.6
        {Rec, 1000, 100000, 0, 0, 1e12, 100000, 1564, 1, -1},    // 1,258,240 columns would fit; 100,000 columns = 1,563 words
        {Dist, 1000, 100000, 0, 0, 1e12, 78640, 78640, 2, -1},   // 157,286,400 / 2,000 = 78,643.2, down to a multiple of 8
        {Occ64, 1, 130, 100, 7, 1e12, 100, -1, 2, 2},
        {Occ64, 1000, 130, 100, 7, 1e12, 100, -1, 2, 2},
        {Occ64, 30000000, 130, 100, 7, 1e12, 100, -1, 2, 2},
    };
    long long n_pins = 0;
    for (const Pin &p : pins) {
        PanelLayout L;
        const int rc = genphi::plan_panels(L, *kRules[p.sweep], p.S, p.n, p.panel, p.group, p.room);
        ++n_pins;
        CHECK(rc == 0, "pin %lld (%s)", n_pins, kNames[p.sweep]);
        CHECK(L.C == p.C && (p.Cp < 0 || L.Cp == p.Cp) && (p.n_panels < 0 || L.n_panels == p.n_panels) && (p.G < 0 || L.per_launch == p.G),
              "pin %lld (%s): C %lld Cp %d n_panels %lld per launch %lld", n_pins, kNames[p.sweep], (long long)L.C, L.Cp, (long long)L.n_panels,
              (long long)L.per_launch);
    }
    std::printf("sweep panels: %lld layouts against the sweeps' own formulas (%lld fit, %lld do not), %lld by hand; %lld violations\n", cases, fit,
                no_fit, n_pins, violations);
    return violations ? 1 : 0;
}
