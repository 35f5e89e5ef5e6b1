// link.cpp -- host side of gen.simuSharing (see link.h): the crossover and transmission words of one (ID, side, simulation) on the
// host, from the same header as the device's step kernel, and genphi_link_words (include/genphi.h); genphi_seg_host, the segments of
// one pair and one simulation by the walk of link_segments.h.  No HIP here.
#include "link.h"

#include <string>

#include "link_segments.h"

#include "../../include/genphi.h"
#include "error.h"

namespace genphi {

static_assert(kLinkMaxLoci == GENPHI_LINK_MAX_LOCI && kLinkMaxQ == GENPHI_LINK_MAX_Q, "link.h and include/genphi.h state the same limits");
static_assert(kSegMaxEdges == GENPHI_SEG_MAX_EDGES && kSegMaxEdge == GENPHI_SEG_MAX_EDGE && kSegMaxGroups == GENPHI_SEG_MAX_GROUPS &&
                  kSegMaxCells == GENPHI_SEG_MAX_CELLS && kSegMaxEdge == kLinkMaxLoci + 1,
              "link_segments.h and include/genphi.h state the same limits");

void link_words(uint64_t seed, int64_t id, int32_t side, uint32_t s, const LinkShape &z, uint64_t *X, uint64_t *T)
{
    const uint64_t uid = static_cast<uint64_t>(id);
    const uint32_t id_lo = static_cast<uint32_t>(uid), id_hi = static_cast<uint32_t>(uid >> 32);
    const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
    uint64_t carry = 0;                      // all ones when the loci before this word hold an odd number of crossovers
    for (int32_t w = 0; w < z.W; ++w) {
        const uint64_t x = link_crossover_word(id_lo, id_hi, s, static_cast<uint32_t>(side), static_cast<uint32_t>(w), static_cast<uint32_t>(z.q), k0, k1);
        const uint64_t t = link_prefix_xor(x) ^ carry;
        if (X) X[w] = x;
        if (T) T[w] = t;
        carry = t >> 63 ? ~0ull : 0ull;
    }
}

}  // namespace genphi

extern "C" int genphi_link_words(uint64_t seed, int64_t id, int32_t side, int64_t s, int32_t loci, int32_t q, uint64_t *X, uint64_t *T)
{
    if (loci < 1 || loci > genphi::kLinkMaxLoci)
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_link_words: loci = " + std::to_string(loci) + " is outside 1 .. 4096");
    if (q < 0 || q > genphi::kLinkMaxQ) return genphi_set_error(GENPHI_ERR_ARG, "genphi_link_words: q = " + std::to_string(q) + " is outside 0 .. 32768");
    if (side != 0 && side != 1) return genphi_set_error(GENPHI_ERR_ARG, "genphi_link_words: side is 0 (from the father) or 1");
    if (s < 0 || s >= GENPHI_SIMU_MAX_SIMULATIONS)
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_link_words: simulation " + std::to_string(s) + " is outside 0 .. 2^24 - 1");
    genphi::link_words(seed, id, side, static_cast<uint32_t>(s), genphi::link_shape(loci, q), X, T);
    return GENPHI_OK;
}

extern "C" int genphi_seg_host(int32_t loci, const uint64_t *any_words, int32_t n_edges, const int32_t *edges, int32_t min_loci, int64_t *hist_out,
                               int64_t *pair_out)
{
    if (loci < 1 || loci > genphi::kLinkMaxLoci)
        return genphi_set_error(GENPHI_ERR_ARG, "genphi_seg_host: loci = " + std::to_string(loci) + " is outside 1 .. 4096");
    if (!any_words) return genphi_set_error(GENPHI_ERR_ARG, "genphi_seg_host: any_words is NULL");
    const std::string err = genphi::seg_check_request(n_edges, edges, min_loci, 0, nullptr, 0);
    if (!err.empty()) return genphi_set_error(GENPHI_ERR_ARG, "genphi_seg_host: " + err);
    genphi::seg_reduce_host(loci, any_words, n_edges, edges, min_loci, hist_out, pair_out);
    return GENPHI_OK;
}
