// cut_format.h -- storage format of the dense level matrices of a Float32 sweep (host and device code; no HIP include, so that
// tests/cut_format_check.cpp builds it with g++).
//
// Every entry of cut c is a multiple of 2^-(2c+1) in [0, 1) (the proof: sparse_levels.h, "Exactness").  While 2c + 1 <= 16 an
// entry is therefore a 16-bit integer in that unit, and while c <= kExactMaxCut a 24-bit one: such a cut may live in HBM as
// those integers instead of as Float32 -- half / three quarters of the bytes, the same values.  A row kernel decodes where it
// writes the staged row to LDS (float(u) * unit: exact) and encodes where it stores its row (v * 2^(2c+1) as an integer: exact),
// so nothing between the two sees a difference.
//
// Which cuts are narrow is a pure function of the plan and its hooks (cut_formats below): a cut is narrow only when the step
// that writes it and the step that reads it both carry the format.
#pragma once
#include <cstdint>
#include <vector>

#include "planner.h"
#include "tuning.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GENPHI_HD __host__ __device__
#else
#define GENPHI_HD
#endif

namespace genphi {

enum CutFormat : int { kFmtF32 = 0, kFmtU16 = 1, kFmtU24 = 2 };

constexpr int kExactMaxCut = 11;              // = kSparseMaxLevel (sparse_levels.h): last cut whose entries are integers below 2^23 in its unit
constexpr int kU16MaxCut = 7;                 // last cut with 2c + 1 <= 16

// The widest narrow format the row kernels are instantiated for (kFmtU16: the 16-bit cuts alone).
constexpr CutFormat kNarrowBuilt = kFmtU24;

GENPHI_HD inline int format_bytes(int fmt) { return fmt == kFmtU16 ? 2 : (fmt == kFmtU24 ? 3 : 4); }
GENPHI_HD inline unsigned format_max(int fmt) { return fmt == kFmtU16 ? 0xffffu : 0x7fffffu; }      // largest integer a narrow entry holds

// one unit of cut c, and its reciprocal (exact powers of two)
GENPHI_HD inline float cut_unit(int c) { return __builtin_ldexpf(1.0f, -(2 * c + 1)); }
GENPHI_HD inline float cut_scale(int c) { return __builtin_ldexpf(1.0f, 2 * c + 1); }

// ---- the encoding: what sparse_dense_kernel and level_split_fast_kernel run, entry by entry and quad by quad ---------------
// decode: exact for u < 2^24
GENPHI_HD inline float decode_entry(unsigned u, float unit) { return static_cast<float>(u) * unit; }

// Float32 -> unsigned, saturating, NaN -> 0: what the GPU's conversion does by itself; the host clamps by hand (the plain
// conversion of a value out of range is undefined there)
GENPHI_HD inline unsigned to_unsigned_sat(float w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<unsigned>(w);
#else
    if (!(w > 0.0f)) return 0u;                             // negative, zero, NaN
    return w >= 4294967296.0f ? 0xffffffffu : static_cast<unsigned>(w);
#endif
}

// The encode guard is a word of bits, != 0 once an entry did not encode exactly; the kernels OR it into a status word of the
// sweep and the host turns it into an error.  It is what makes a wrong eligibility rule loud; on a cut the rule allows it stays 0.
//   encode_bits   v * scale as an integer (exact product: a power of two).  Guard: the bits of float(u) - w without the sign --
//                 0 only when w is that integer (+-0 both give +0); a fraction, a negative value, NaN and infinity all leave bits
//   range_bits    `any` = the OR of the integers of a quad (or one of them): the bits a narrow entry cannot hold
GENPHI_HD inline unsigned encode_bits(float v, float scale, unsigned &gbad)
{
    const float w = v * scale;
    const unsigned u = to_unsigned_sat(w);
    gbad |= __builtin_bit_cast(unsigned, static_cast<float>(u) - w) << 1;
    return u;
}
GENPHI_HD inline unsigned range_bits(unsigned any, int fmt) { return any >> (fmt == kFmtU16 ? 16 : 23); }

// four consecutive entries of a 16-bit row: two words; of a 24-bit row: three words, entries packed little endian (bytes 3k .. 3k + 2
// hold entry k), so that a quad of columns is one aligned 8- / 12-byte access
struct Quad16 { unsigned x, y; };
struct Quad24 { unsigned x, y, z; };
GENPHI_HD inline Quad16 pack_quad16(unsigned a, unsigned b, unsigned c, unsigned d) { return Quad16{a | (b << 16), c | (d << 16)}; }
GENPHI_HD inline Quad24 pack_quad24(unsigned a, unsigned b, unsigned c, unsigned d)
{
    return Quad24{a | (b << 24), (b >> 8) | (c << 16), (c >> 16) | (d << 8)};
}
GENPHI_HD inline void unpack_quad(const Quad16 &q, unsigned u[4]) { u[0] = q.x & 0xffffu; u[1] = q.x >> 16; u[2] = q.y & 0xffffu; u[3] = q.y >> 16; }
GENPHI_HD inline void unpack_quad(const Quad24 &q, unsigned u[4])
{
    u[0] = q.x & 0xffffffu; u[1] = (q.x >> 24) | ((q.y & 0xffffu) << 8); u[2] = (q.y >> 16) | ((q.z & 0xffu) << 16); u[3] = q.z >> 8;
}

// a quad of values of the cut written, encoded and packed; the guard of all four goes to gbad
GENPHI_HD inline Quad16 encode_quad16(float a, float b, float c, float d, float scale, unsigned &gbad)
{
    const unsigned u0 = encode_bits(a, scale, gbad), u1 = encode_bits(b, scale, gbad), u2 = encode_bits(c, scale, gbad), u3 = encode_bits(d, scale, gbad);
    gbad |= range_bits(u0 | u1 | u2 | u3, kFmtU16);
    return pack_quad16(u0, u1, u2, u3);
}
GENPHI_HD inline Quad24 encode_quad24(float a, float b, float c, float d, float scale, unsigned &gbad)
{
    const unsigned u0 = encode_bits(a, scale, gbad), u1 = encode_bits(b, scale, gbad), u2 = encode_bits(c, scale, gbad), u3 = encode_bits(d, scale, gbad);
    gbad |= range_bits(u0 | u1 | u2 | u3, kFmtU24);
    return pack_quad24(u0, u1, u2, u3);
}
// one entry (the diagonal patch), with its range check
GENPHI_HD inline unsigned encode_one(float v, float scale, int fmt, unsigned &gbad)
{
    const unsigned u = encode_bits(v, scale, gbad);
    gbad |= range_bits(u, fmt);
    return u;
}

// ---- the rule ----------------------------------------------------------------------------------------------------------
// What a level step of a sweep is, as far as formats go.  Only two kinds write a narrow cut and only one reads one.
enum StepKind : int {
    kStepFast = 0,          // SPLIT step on the certified-rows kernel, default run lists (CHAIN = false): reads and writes narrow cuts
    kStepSparseDense,       // the row lists -> dense matrix step of a Float32 sweep, compact rows: writes narrow cuts
    kStepSparseList,        // a row-list step: neither reads nor writes a matrix
    kStepFull, kStepWide, kStepInPlace, kStepIdentity, kStepSmall,
    kStepExact,             // SPLIT step that may run the grouping-exact kernel (GENPHI_NO_FAST, a raised certificate bound, chain steps)
    kStepNaive,             // kernel = 1
    kStepProband,           // the last step: writes the proband cut
};
// (the Float64-storage sweep and the column panels never come here: they have sweeps of their own, which know Float32 / Float64 only)

inline bool step_writes_narrow(int kind) { return kind == kStepFast || kind == kStepSparseDense; }
inline bool step_reads_narrow(int kind) { return kind == kStepFast; }

// Format of cut c, written by a step of kind `writer` whose own source has format `writer_src` and read by a step of kind
// `reader`; `widest` = the widest narrow format the kernels carry (kFmtF32: none).  A certified-rows step starts no narrow run:
// it writes a narrow cut only when it reads one (the run starts at the sparse -> dense step), which keeps the (source,
// destination) pairs to u16 -> u16, u16 -> u24, u24 -> u24 and narrow -> f32.
inline CutFormat cut_format(int c, int writer, int writer_src, int reader, CutFormat widest)
{
    if (widest == kFmtF32 || c < 1 || !step_writes_narrow(writer) || !step_reads_narrow(reader)) return kFmtF32;
    if (writer == kStepFast && writer_src == kFmtF32) return kFmtF32;
    if (c <= kU16MaxCut) return kFmtU16;
    if (c <= kExactMaxCut && widest == kFmtU24) return kFmtU24;
    return kFmtF32;
}

// Formats of cuts 0 .. n_steps (cut c is written by step c - 1 and read by step c; cut 0 and the proband cut are never narrow)
// from the kinds of steps 0 .. n_steps - 1.
inline std::vector<int> cut_formats(const std::vector<int> &kinds, CutFormat widest)
{
    const int n_steps = static_cast<int>(kinds.size());
    std::vector<int> fmt(static_cast<size_t>(n_steps) + 1, kFmtF32);
    for (int c = 1; c < n_steps; ++c) fmt[c] = cut_format(c, kinds[c - 1], fmt[c - 1], kinds[c], widest);
    return fmt;
}


// Kinds of the steps of a plan's Float32 sweep: kernel = opts.kernel, sparse_k = the last cut kept as row lists (-1: none),
// small_max = the widest cut of the fused small-level kernel.  Conservative where a step MAY take a path without narrow forms
// (a small step counts as one whether or not its run is long enough to be fused).
inline std::vector<int> sweep_step_kinds(const Plan &pl, const Tuning &tun, int kernel, int sparse_k, int small_max)
{
    const int n_steps = pl.n_levels - 1;
    std::vector<int> kinds(static_cast<size_t>(n_steps > 0 ? n_steps : 0), kStepFull);
    for (int s = 0; s < n_steps; ++s) {
        const LevelStep &st = pl.steps[s];
        int k;
        if (s < sparse_k) k = kStepSparseList;
        else if (s == sparse_k) k = (kernel == 0 && !st.stay && !st.src_slots) ? kStepSparseDense : kStepInPlace;
        else if (kernel != 0) k = kStepNaive;
        else if (s == n_steps - 1) k = kStepProband;
        else if (s == 0 && !tun.no_identity) k = kStepIdentity;
        else if (st.stay || st.src_slots) k = kStepInPlace;
        else if (st.mode == kModeWide) k = kStepWide;
        else if (!tun.no_small && st.n_prev <= small_max && st.n <= small_max) k = kStepSmall;
        else if (st.mode == kModeFull) k = kStepFull;
        else if (st.mode == kModeSplit) k = (tun.no_fast || tun.max_run > 1 || tun.cert_min_exp > -27) ? kStepExact : kStepFast;
        else k = kStepFull;
        kinds[s] = k;
    }
    return kinds;
}

}  // namespace genphi
