// pedigree_index.cpp -- ID -> rank, the parents' ranks and the probands' ranks of a pedigree (see pedigree_index.h).
#include "pedigree_index.h"

#include <utility>

#include "../../include/genphi.h"

namespace genphi {

namespace {

// (out of the loop below: the message of a row that is refused)
int order_error(std::string &err, int64_t id, const char *which, int64_t parent)
{
    err = "individual " + std::to_string(id) + ": " + which + " " + std::to_string(parent) +
          " is unknown or listed after its child (pedigree must be in rank order)";
    return GENPHI_ERR_ORDER;
}

}  // namespace

int index_pedigree(PedigreeIndex &out, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, std::string &err)
{
    Ranks ranks;
    ranks.init(n_ind, ind);
    std::vector<int32_t> fa(n_ind, -1), mo(n_ind, -1);
    for (int64_t i = 0; i < n_ind; ++i) {
        // (the direct table keeps the last rank of an ID, the map the first: either way a copy's rank is not its own)
        if (ranks.find(ind[i]) != i) { err = "duplicate individual ID " + std::to_string(ind[i]); return GENPHI_ERR_DUPLICATE_ID; }
        if (father[i] != 0) {
            fa[i] = ranks.find(father[i]);
            if (fa[i] < 0 || fa[i] >= i) return order_error(err, ind[i], "father", father[i]);
        }
        if (mother[i] != 0) {
            mo[i] = ranks.find(mother[i]);
            if (mo[i] < 0 || mo[i] >= i) return order_error(err, ind[i], "mother", mother[i]);
        }
    }
    out.ranks = std::move(ranks);
    out.fa = std::move(fa);
    out.mo = std::move(mo);
    return GENPHI_OK;
}

int find_probands(std::vector<int32_t> &pro_rank, const Ranks &ranks, int64_t n_pro, const int64_t *pro_ids, std::string &err)
{
    pro_rank.resize(n_pro);
    for (int64_t k = 0; k < n_pro; ++k) {
        pro_rank[k] = ranks.find(pro_ids[k]);
        if (pro_rank[k] < 0) { err = "KeyError: proband " + std::to_string(pro_ids[k]) + " not found"; return GENPHI_ERR_UNKNOWN_ID; }
    }
    return GENPHI_OK;
}

}  // namespace genphi
