// depth_word.h -- the row element of gen.depths (csrc/depth.hip): the word arithmetic of its recursion, plain C++ for host and
// device (tests/depth_check.cpp runs it on the CPU).
//
// For a row x and an ancestor column j, over all ascending paths from x to ancestors[j] (length = meioses; the empty path counts
// where x is the ancestor):  P = their number, S = the sum of their lengths, min / max = the shortest / longest length.
//     P[x] = P[f] + P[m],   S[x] = S[f] + S[m] + P[x],   min[x] = min(min[f], min[m]) + 1,   max[x] = max(max[f], max[m]) + 1
// ("none" is absorbing, a missing parent is none), then P = 1, S = 0, min = max = 0 where ancestors[j] == x.
//
// Encoding: 16 bytes, and the zero element is "none" (in the schedule the row of an unrelated member, a missing parent and a member
// that is never computed are all the zero row):
//     word 0   P in bits 0-47,  the closeness 255 - min in bits 48-55 (0 = none),  max + 1 in bits 56-63 (0 = none)
//     word 1   S as Int64
//
// The bound GENPHI_DEPTH_MAX_STEPS = 47.  The paths from x to one ancestor, written as strings of father / mother choices, form a
// prefix-free set of binary strings (a path ends where it reaches the ancestor, so no path extends another): by Kraft's inequality
// sum 2^-length <= 1, and with every length <= L that gives P <= 2^L.  L <= n_steps, the level steps of the sweep (the bound dist.hip
// uses for min; tests/depth_check.cpp asserts it on every row).  With L <= 47:
//     P <= 2^47 fits 48 bits, and the sum of two packed P fields of parents (each <= 2^46 where the child's is <= 2^47) never
//         carries into bit 48;
//     S <= 47 * 2^47 < 2^53, so double(S) / double(P) is the correctly rounded mean of exact operands;
//     min, max <= 47: the closeness stays >= 208 and max + 1 <= 48, a byte each.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GENPHI_DEPTH_HD __host__ __device__
#else
#define GENPHI_DEPTH_HD
#endif

#ifndef GENPHI_DEPTH_MAX_STEPS
#define GENPHI_DEPTH_MAX_STEPS 47      // (include/genphi.h defines the same value)
#endif

namespace genphi {

struct alignas(16) DepthWord {
    uint64_t w;      // P | closeness << 48 | (max + 1) << 56
    int64_t s;       // S
};

constexpr uint64_t kDepthPathMask = (uint64_t(1) << 48) - 1;
constexpr unsigned kDepthNear = 255;      // the closeness of an individual to itself

GENPHI_DEPTH_HD inline uint64_t depth_paths(const DepthWord &v) { return v.w & kDepthPathMask; }
GENPHI_DEPTH_HD inline unsigned depth_close(const DepthWord &v) { return static_cast<unsigned>(v.w >> 48) & 255u; }
GENPHI_DEPTH_HD inline unsigned depth_far(const DepthWord &v) { return static_cast<unsigned>(v.w >> 56); }

GENPHI_DEPTH_HD inline DepthWord depth_pack(uint64_t paths, unsigned close, unsigned far, int64_t sum)
{
    return DepthWord{paths | (static_cast<uint64_t>(close) << 48) | (static_cast<uint64_t>(far) << 56), sum};
}

// x itself is the ancestor of this column: one path of no meiosis
GENPHI_DEPTH_HD inline DepthWord depth_onehot() { return depth_pack(1, kDepthNear, 1, 0); }

// The element of a child from its parents' (a missing parent: the zero element).  step = 1; step = 0 for a copy item of the last
// list (b is then the zero element and a is returned as it is).
GENPHI_DEPTH_HD inline DepthWord depth_step(const DepthWord &a, const DepthWord &b, unsigned step)
{
    const uint64_t paths = (a.w + b.w) & kDepthPathMask;                  // (no carry out of the P fields: see above)
    const unsigned ca = depth_close(a), cb = depth_close(b), fa = depth_far(a), fb = depth_far(b);
    const unsigned c = ca > cb ? ca : cb, f = fa > fb ? fa : fb;          // the shorter of the shortest, the longer of the longest
    const int64_t sum = a.s + b.s + (step ? static_cast<int64_t>(paths) : 0);
    return depth_pack(paths, c ? c - step : 0, f ? f + step : 0, sum);    // none (c = f = 0, P = 0, S = 0) stays none
}

// what the result holds
GENPHI_DEPTH_HD inline int16_t depth_min_of(unsigned close) { return close ? static_cast<int16_t>(kDepthNear - close) : int16_t(-1); }
GENPHI_DEPTH_HD inline int16_t depth_max_of(unsigned far) { return far ? static_cast<int16_t>(far - 1) : int16_t(-1); }
// the mean length: exact operands (S < 2^53, P < 2^53), one rounding; NaN where there is no path
GENPHI_DEPTH_HD inline double depth_mean_of(uint64_t paths, int64_t sum)
{
    return paths ? static_cast<double>(sum) / static_cast<double>(paths) : __builtin_nan("");
}

}  // namespace genphi
