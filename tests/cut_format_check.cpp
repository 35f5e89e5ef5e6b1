// cut_format_check.cpp -- csrc/cut_format.h without a GPU: the format rule (which cuts of a sweep are kept as 16- / 24-bit integers),
// the encoding both sides of a narrow cut share, its guard, and what the narrow forms of the certified-rows kernel add to the
// invariants of tests/row_geometry_check.cpp.  Built with g++ (and once more under AddressSanitizer + UndefinedBehaviorSanitizer).
//
//   g++ -std=c++17 -O2 tests/cut_format_check.cpp -o cut_format_check && ./cut_format_check
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../genlib.jl_amd/csrc/cut_format.h"
#include "../genlib.jl_amd/csrc/device_sizes.h"
#include "../genlib.jl_amd/csrc/row_geometry.h"

using namespace genphi;

static long long g_checks = 0, g_violations = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_violations; if (g_violations < 40) std::fprintf(stderr, "VIOLATION line %d: %s\n", __LINE__, #cond); } } while (0)

static const int kAllKinds[] = {kStepFast, kStepSparseDense, kStepSparseList, kStepFull, kStepWide, kStepInPlace, kStepIdentity, kStepSmall,
                                kStepExact, kStepNaive, kStepProband};

static void check_rule()
{
    // the table: (cut, writer, format of the writer's source, reader, widest format built) -> format
    for (int c = 0; c <= 14; ++c)
        for (int w : kAllKinds)
            for (int r : kAllKinds)
                for (int ws : {kFmtF32, kFmtU16, kFmtU24})
                    for (CutFormat widest : {kFmtF32, kFmtU16, kFmtU24}) {
                        const CutFormat f = cut_format(c, w, ws, r, widest);
                        const bool writer_ok = w == kStepSparseDense || (w == kStepFast && ws != kFmtF32);
                        const bool pair_ok = writer_ok && r == kStepFast && c >= 1 && widest != kFmtF32;
                        CutFormat want = kFmtF32;
                        if (pair_ok && 2 * c + 1 <= 16) want = kFmtU16;
                        else if (pair_ok && c <= 11 && widest == kFmtU24) want = kFmtU24;
                        CHECK(f == want);
                    }
    // both boundaries
    CHECK(cut_format(7, kStepFast, kFmtU16, kStepFast, kFmtU24) == kFmtU16 && cut_format(8, kStepFast, kFmtU16, kStepFast, kFmtU24) == kFmtU24);
    CHECK(cut_format(11, kStepFast, kFmtU24, kStepFast, kFmtU24) == kFmtU24 && cut_format(12, kStepFast, kFmtU24, kStepFast, kFmtU24) == kFmtF32);
    CHECK(cut_format(7, kStepSparseDense, kFmtF32, kStepFast, kFmtU16) == kFmtU16 && cut_format(8, kStepSparseDense, kFmtF32, kStepFast, kFmtU16) == kFmtF32);
    CHECK(kU16MaxCut == 7 && kExactMaxCut == 11 && 2 * kU16MaxCut + 1 <= 16 && 2 * (kU16MaxCut + 1) + 1 > 16 && 2 * kExactMaxCut + 1 <= 23);
    // every excluded kind, as the writer and as the reader of a cut that two certified-rows steps would keep narrow
    for (int k : kAllKinds) {
        if (k != kStepFast) CHECK(cut_format(5, kStepFast, kFmtU16, k, kFmtU24) == kFmtF32);
        if (k != kStepFast && k != kStepSparseDense) CHECK(cut_format(5, k, kFmtU16, kStepFast, kFmtU24) == kFmtF32);
        CHECK(step_reads_narrow(k) == (k == kStepFast) && step_writes_narrow(k) == (k == kStepFast || k == kStepSparseDense));
    }
    // a sweep: lists up to cut 3, the sparse -> dense step, certified-rows steps, the proband step
    {
        std::vector<int> kinds = {kStepSparseList, kStepSparseList, kStepSparseList, kStepSparseDense};
        for (int s = 4; s < 15; ++s) kinds.push_back(kStepFast);
        kinds.push_back(kStepProband);
        const std::vector<int> f16 = cut_formats(kinds, kFmtU16), f24 = cut_formats(kinds, kFmtU24), f32 = cut_formats(kinds, kFmtF32);
        CHECK(f16.size() == kinds.size() + 1);
        for (int c = 0; c <= 16; ++c) {
            CHECK(f16[c] == (c >= 4 && c <= 7 ? kFmtU16 : kFmtF32));
            CHECK(f24[c] == (c >= 4 && c <= 7 ? kFmtU16 : (c >= 8 && c <= 11 ? kFmtU24 : kFmtF32)));
            CHECK(f32[c] == kFmtF32);
        }
        // a Float32 step in the middle ends the run for good: a certified-rows step starts none
        kinds[6] = kStepFull;
        const std::vector<int> g = cut_formats(kinds, kFmtU24);
        for (int c = 0; c <= 16; ++c) CHECK(g[c] == (c >= 4 && c <= 5 ? kFmtU16 : kFmtF32));
        // no list cuts: every cut Float32
        std::vector<int> dense(12, kStepFast);
        dense[0] = kStepIdentity; dense[11] = kStepProband;
        for (int f : cut_formats(dense, kFmtU24)) CHECK(f == kFmtF32);
        // the last list cut too late for 16 bits
        std::vector<int> late = {kStepSparseList, kStepSparseList, kStepSparseList, kStepSparseList, kStepSparseList, kStepSparseList, kStepSparseList,
                                 kStepSparseDense, kStepFast, kStepFast, kStepFast, kStepFast, kStepFast, kStepProband};
        const std::vector<int> l16 = cut_formats(late, kFmtU16), l24 = cut_formats(late, kFmtU24);
        for (int c = 0; c <= 13; ++c) { CHECK(l16[c] == kFmtF32); CHECK(l24[c] == (c >= 8 && c <= 11 ? kFmtU24 : kFmtF32)); }
    }
    // the kinds of a plan's steps from the plan and its hooks
    {
        Plan pl;
        pl.n_levels = 12;
        pl.steps.resize(11);
        for (int s = 0; s < 11; ++s) { pl.steps[s].n_prev = 3000 + s; pl.steps[s].n = 3001 + s; pl.steps[s].mode = kModeSplit; }
        Tuning tun;
        std::vector<int> k = sweep_step_kinds(pl, tun, 0, 3, 128);
        CHECK(k.size() == 11 && k[0] == kStepSparseList && k[2] == kStepSparseList && k[3] == kStepSparseDense && k[4] == kStepFast && k[9] == kStepFast &&
              k[10] == kStepProband);
        k = sweep_step_kinds(pl, tun, 0, -1, 128);
        CHECK(k[0] == kStepIdentity && k[1] == kStepFast);
        tun.no_identity = true;
        CHECK(sweep_step_kinds(pl, tun, 0, -1, 128)[0] == kStepFast);
        CHECK(sweep_step_kinds(pl, tun, 1, -1, 128)[4] == kStepNaive && sweep_step_kinds(pl, tun, 1, 3, 128)[3] == kStepInPlace);
        Tuning t2; t2.no_fast = true;
        CHECK(sweep_step_kinds(pl, t2, 0, 3, 128)[5] == kStepExact);
        Tuning t3; t3.max_run = 4;
        CHECK(sweep_step_kinds(pl, t3, 0, 3, 128)[5] == kStepExact);
        Tuning t4; t4.cert_min_exp = -9;
        CHECK(sweep_step_kinds(pl, t4, 0, 3, 128)[5] == kStepExact);
        Tuning t5; t5.cert_min_exp = -40;                      // (clamped to the default bound)
        CHECK(sweep_step_kinds(pl, t5, 0, 3, 128)[5] == kStepFast);
        pl.steps[5].mode = kModeFull; pl.steps[6].mode = kModeWide; pl.steps[7].stay = true; pl.steps[8].src_slots = true; pl.steps[3].stay = true;
        pl.steps[9].n_prev = 100; pl.steps[9].n = 128;
        k = sweep_step_kinds(pl, Tuning(), 0, 3, 128);
        CHECK(k[3] == kStepInPlace && k[5] == kStepFull && k[6] == kStepWide && k[7] == kStepInPlace && k[8] == kStepInPlace && k[9] == kStepSmall);
        Tuning t6; t6.no_small = true;
        CHECK(sweep_step_kinds(pl, t6, 0, 3, 128)[9] == kStepFast);
        Plan none;
        none.n_levels = 1;
        CHECK(sweep_step_kinds(none, Tuning(), 0, -1, 128).empty() && cut_formats({}, kFmtU24).size() == 1);
    }
}

// The functions below are the ones sparse_dense_kernel and level_split_fast_kernel call (GENPHI_HD in cut_format.h): a quad is encoded,
// packed, unpacked and decoded here exactly as on the device, and the guard word is the kernels' guard word.
template <typename Q>
static Q encode_quad(const float v[4], float scale, unsigned &gbad);
template <>
Quad16 encode_quad<Quad16>(const float v[4], float scale, unsigned &gbad) { return encode_quad16(v[0], v[1], v[2], v[3], scale, gbad); }
template <>
Quad24 encode_quad<Quad24>(const float v[4], float scale, unsigned &gbad) { return encode_quad24(v[0], v[1], v[2], v[3], scale, gbad); }

// integers u[4] of cut c through decode -> encode_quad -> unpack -> decode: the same integers, the same Float32 values, guard 0
template <typename Q>
static void round_trip(const unsigned u[4], int c, int fmt)
{
    const float unit = cut_unit(c), scale = cut_scale(c);
    float v[4];
    for (int e = 0; e < 4; ++e) {
        v[e] = decode_entry(u[e], unit);
        CHECK(static_cast<double>(v[e]) == std::ldexp(static_cast<double>(u[e]), -(2 * c + 1)));
    }
    unsigned gbad = 0u, back[4];
    const Q q = encode_quad<Q>(v, scale, gbad);
    unpack_quad(q, back);
    CHECK(gbad == 0u && back[0] == u[0] && back[1] == u[1] && back[2] == u[2] && back[3] == u[3]);
    for (int e = 0; e < 4; ++e) {
        unsigned g1 = 0u;
        CHECK(decode_entry(back[e], unit) == v[e] && encode_one(v[e], scale, fmt, g1) == u[e] && g1 == 0u);
    }
}

// v in position `pos` of an otherwise good quad fires the guard, whatever it is combined with, and the guard is never cleared
template <typename Q>
static void guard_fires(float v, int c, int fmt)
{
    const float unit = cut_unit(c), scale = cut_scale(c);
    for (int pos = 0; pos < 4; ++pos) {
        float q[4] = {unit, 0.0f, 3.0f * unit, 0.5f};
        q[pos] = v;
        unsigned gbad = 0u;
        (void)encode_quad<Q>(q, scale, gbad);
        CHECK(gbad != 0u);
        const float good[4] = {unit, 0.0f, 3.0f * unit, 0.5f};
        (void)encode_quad<Q>(good, scale, gbad);
        CHECK(gbad != 0u);
    }
    unsigned g1 = 0u;
    (void)encode_one(v, scale, fmt, g1);
    CHECK(g1 != 0u);
    (void)encode_one(unit, scale, fmt, g1);
    CHECK(g1 != 0u);
}

static void check_codec()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // the conversion: saturating, NaN and negative values to 0 (the host's clamp states what the GPU's conversion does)
    CHECK(to_unsigned_sat(0.0f) == 0u && to_unsigned_sat(-0.0f) == 0u && to_unsigned_sat(-3.0f) == 0u && to_unsigned_sat(nan) == 0u && to_unsigned_sat(-inf) == 0u);
    CHECK(to_unsigned_sat(65535.0f) == 65535u && to_unsigned_sat(8388607.0f) == 8388607u && to_unsigned_sat(2.75f) == 2u);
    CHECK(to_unsigned_sat(4294967296.0f) == 0xffffffffu && to_unsigned_sat(1e30f) == 0xffffffffu && to_unsigned_sat(inf) == 0xffffffffu && to_unsigned_sat(4294967040.0f) == 4294967040u);
    CHECK(range_bits(65535u, kFmtU16) == 0u && range_bits(65536u, kFmtU16) != 0u && range_bits(0x7fffffu, kFmtU24) == 0u && range_bits(0x800000u, kFmtU24) != 0u &&
          range_bits(0xffffffffu, kFmtU16) != 0u && range_bits(0xffffffffu, kFmtU24) != 0u);
    // 16 bits: every one of the 65,536 values of every cut that may be kept so, in every position of a quad
    for (int c = 0; c <= kU16MaxCut; ++c) {
        CHECK(cut_unit(c) * cut_scale(c) == 1.0f && cut_unit(c) == std::ldexp(1.0f, -(2 * c + 1)));
        for (unsigned u = 0; u < 65536u; ++u) {
            const unsigned q[4] = {u, 65535u - u, (u * 40503u) & 0xffffu, (u + 1u) & 0xffffu};
            round_trip<Quad16>(q, c, kFmtU16);
        }
    }
    // 24 bits: the ends, a stride through the range, and per cut the largest entry and the largest diagonal the recursion can produce
    // (an entry is < 1: 2^(2c+1) - 1 units; a diagonal is 1/2 + Psi/2 with Psi an entry of cut c - 1: 2^(2c+1) - 2 units)
    for (int c = 6; c <= kExactMaxCut; ++c) {
        const float unit = cut_unit(c), scale = cut_scale(c);
        std::vector<unsigned> vals = {0u, 1u, 0x7fffffu, (1u << (2 * c + 1)) - 1u, (1u << (2 * c + 1)) - 2u, 1u << (2 * c), 0x555555u, 0x2aaaaau, 0x7f00ffu, 0x00ff00u};
        for (unsigned u = 0; u < (1u << 23); u += 4099u) vals.push_back(u);
        for (size_t k = 0; k < vals.size(); ++k) {
            const unsigned q[4] = {vals[k], vals[(k + 1) % vals.size()], 0x7fffffu - vals[k], vals[(k * 7 + 3) % vals.size()]};
            round_trip<Quad24>(q, c, kFmtU24);
        }
        const double prev_max = 1.0 - std::ldexp(1.0, -(2 * c - 1));                          // largest entry of cut c - 1
        const float diag = static_cast<float>(0.5 + 0.5 * prev_max);                          // as the row kernels compute it
        unsigned gbad = 0u;
        CHECK(encode_one(diag, scale, kFmtU24, gbad) == (1u << (2 * c + 1)) - 2u && gbad == 0u && decode_entry((1u << (2 * c + 1)) - 2u, unit) == diag);
    }
    // the packing itself: entry k of a 24-bit quad is bytes 3k .. 3k + 2, of a 16-bit quad bytes 2k .. 2k + 1, little endian
    {
        const Quad24 q = pack_quad24(0x030201u, 0x060504u, 0x090807u, 0x0c0b0au);
        CHECK(q.x == 0x04030201u && q.y == 0x08070605u && q.z == 0x0c0b0a09u);
        const Quad16 h = pack_quad16(0x0201u, 0x0403u, 0x0605u, 0x0807u);
        CHECK(h.x == 0x04030201u && h.y == 0x08070605u);
    }
    CHECK(format_bytes(kFmtF32) == 4 && format_bytes(kFmtU16) == 2 && format_bytes(kFmtU24) == 3 && format_max(kFmtU16) == 65535u && format_max(kFmtU24) == 8388607u);
    // the guard: no multiple of the unit, past the range, negative, not a number, infinite -- and it is never cleared
    for (int c : {1, 6, 7}) {
        const float unit = cut_unit(c);
        for (float v : {unit * 0.5f, unit * 1.5f, unit * 0.999f, std::ldexp(1.0f, -30), 0.3f, -unit, -0.3f, nan, 65536.0f * unit, 65537.0f * unit, 1e30f, inf, -inf})
            guard_fires<Quad16>(v, c, kFmtU16);
        unsigned ok = 0u;
        CHECK(encode_one(65535.0f * unit, cut_scale(c), kFmtU16, ok) == 65535u && ok == 0u);
        CHECK(encode_one(-0.0f, cut_scale(c), kFmtU16, ok) == 0u && ok == 0u);                  // (-0 is 0)
    }
    for (int c : {8, 11}) {
        const float unit = cut_unit(c);
        for (float v : {unit * 0.5f, unit * 1.25f, 8388608.0f * unit, 8388610.0f * unit, 16777216.0f * unit, -unit, nan, 1e30f, inf, -inf})
            guard_fires<Quad24>(v, c, kFmtU24);
        unsigned ok = 0u;
        CHECK(encode_one(8388607.0f * unit, cut_scale(c), kFmtU24, ok) == 8388607u && ok == 0u);
    }
}

// the hook: GENPHI_NO_NARROW is known, read like the others, off by default, and sits in a list of its own (tuning.h says why)
static void check_hook()
{
    CHECK(tuning_knows("GENPHI_NO_NARROW") && !tuning_knows("NO_NARROW") && !tuning_knows("GENPHI_NO_NARROW "));
    genphi_tuning none, on, off;
    on.kv["GENPHI_NO_NARROW"] = "1";
    off.kv["GENPHI_NO_NARROW"] = "0";
    CHECK(!Tuning().no_narrow && !tuning_from(&none).no_narrow && tuning_from(&on).no_narrow && !tuning_from(&off).no_narrow);
    on.kv["GENPHI_FAST_NT"] = "512";                           // (both lists are read)
    CHECK(tuning_from(&on).no_narrow && tuning_from(&on).fast_nt == 512);
#define COUNT(NAME, SET) +1
    CHECK((0 GENPHI_FORMAT_HOOKS(COUNT)) == 1);
#undef COUNT
}

// what the narrow forms add to row_geometry_check.cpp: the same instantiation list and geometry serve them, so what is left to hold is the
// pair list and the bytes a narrow row is staged from
static void check_narrow_forms()
{
    CHECK(kNumNarrowPairs >= 1 && fast_form_built(kFmtF32, 512) && fast_form_built(kFmtU16, 512) && !fast_form_built(kFmtU24, 512) && fast_form_built(kFmtU24, 1024));
    for (int i = 0; i < kNumNarrowPairs; ++i) {
        const NarrowPair &p = kNarrowPairs[i];
        CHECK(p.sf != kFmtF32 && p.sf <= kNarrowBuilt && p.df <= kNarrowBuilt && kNarrowBuilt == kFmtU24);                 // a narrow run starts at the sparse -> dense step
        CHECK(p.df == kFmtF32 || p.df >= p.sf);                                                 // formats only widen along a sweep
        CHECK(narrow_pair_index(p.sf, p.df) == i);
    }
    CHECK(narrow_pair_index(kFmtF32, kFmtF32) < 0 && narrow_pair_index(kFmtF32, kFmtU16) < 0 && narrow_pair_index(kFmtF32, kFmtU24) < 0);
    // every pair the rule can produce with the formats built has its forms
    for (int sf = kFmtU16; sf <= kNarrowBuilt; ++sf) {
        CHECK(narrow_pair_index(sf, sf) >= 0 && narrow_pair_index(sf, kFmtF32) >= 0);
        for (int df = sf + 1; df <= kNarrowBuilt; ++df) CHECK(narrow_pair_index(sf, df) >= 0);
    }
    for (int i = 0; i < kNumFastInsts; ++i) {
        const FastInst &f = kFastInsts[i];
        // a thread stages STG quads of 8 / 12 bytes: the unconditional loads past the end of the last row stay inside the zeroed tail of a level buffer
        CHECK(static_cast<size_t>(f.stg) * f.nt * 12u <= kTailPadFloats * sizeof(float));
        CHECK(f.c % 4 == 0);                                                                    // rows are stored in whole quads (8 / 12 bytes of a narrow row)
    }
    // rows of a narrow cut start on 16-byte boundaries: the pitch is a multiple of 64 entries
    for (int64_t n : {1, 63, 64, 127, 4111, 4112, 24300, 65534}) {
        CHECK(pitch_for(n) % 64 == 0);
        for (int fmt : {kFmtU16, kFmtU24}) CHECK(pitch_for(n) * format_bytes(fmt) % 16 == 0);
    }
    // a narrow source changes nothing in the geometry: it is the Float32 form's, and the dispatch finds an instantiation for it
    // ... except that a 24-bit source keeps to the 1024-thread forms, GENPHI_FAST_NT or not: its 512-thread forms are not built
    Tuning tun, t512;
    t512.fast_nt = 512;
    for (int64_t n_prev : {600, 4112, 24300, 30000, 36000})
        for (int64_t width : {640, 4160, 24320, 24640, 28672, 30016, 36864})
            for (int fmt : {kFmtF32, kFmtU16, kFmtU24}) {
                const SplitGeometry g = split_geometry(n_prev + 1, width, false, 0, true, 256, 100, 50, tun, false, fmt);
                const SplitGeometry g32 = split_geometry(n_prev + 1, width, false, 0, true, 256, 100, 50, tun, false);
                CHECK(g.certs && !g.chain && fast_inst_for(g.fast.nt, g.fast.cpt, g.fast.stg) >= 0 && fast_form_built(fmt, g.fast.nt));
                CHECK(static_cast<int64_t>(g.fast.stg) * g.fast.nt * 4 >= g.lds_row);            // the staged quads cover the row, in entries
                CHECK(static_cast<int64_t>(g.fast.chunk_cols) * g.fast.n_chunks >= width);
                if (fmt != kFmtU24) CHECK(g.fast.nt == g32.fast.nt && g.fast.cpt == g32.fast.cpt && g.fast.stg == g32.fast.stg && g.fast.n_chunks == g32.fast.n_chunks);
                else CHECK(g.fast.nt == 1024 && g.fast.n_chunks >= g32.fast.n_chunks);
                const SplitGeometry g512 = split_geometry(n_prev + 1, width, false, 0, true, 256, 100, 50, t512, false, fmt);
                CHECK(g512.fast.nt == (fmt == kFmtU24 ? 1024 : 512) && fast_form_built(fmt, g512.fast.nt) && fast_inst_for(g512.fast.nt, g512.fast.cpt, g512.fast.stg) >= 0);
                if (fmt == kFmtU24) CHECK(g512.fast.cpt == g.fast.cpt && g512.fast.n_chunks == g.fast.n_chunks);
            }
}

int main()
{
    check_rule();
    check_codec();
    check_hook();
    check_narrow_forms();
    std::printf("cut format check: %lld checks; %lld violations\n", g_checks, g_violations);
    return g_violations ? 1 : 0;
}
