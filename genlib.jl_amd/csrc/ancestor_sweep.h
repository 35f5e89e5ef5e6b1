// ancestor_sweep.h -- host schedule of the ancestor x proband sweeps (gen.gc, gen.occ, gen.rec, gen.meioses) and of the
// generation x proband sweep of gen.completeness (SweepOptions::every_member); no HIP here.
//
// The first four are column-independent recursions over the generation cuts of the planner (build_plan, indices_only):
//     row[x] = combine(row[father], row[mother])   (a missing parent is the zero row),   then the one-hot columns j with
//     ancestors[j] == x are set / incremented
// and share everything but the arithmetic and the rule that says which rows reach the result:
//   rows    only members that are a requested ancestor or descend from one are computed; every other row is zero ("none")
//   slots   each computed member owns one row of a slot buffer from the step that creates it until its last cut has been
//           read; members dragged from one cut to the next keep their slot (nothing is copied); a slot freed after step s is
//           handed out from step s+1 on, never inside the launch that still reads it
//   emit    Emit::LeafFirst     (gc)  the last step writes straight into the result: only the first occurrence of a LEAF
//                                     proband (no children anywhere in the pedigree) gets a row
//           Emit::EveryProband  (occ) the last step writes one result row for EVERY occurrence of every proband with a
//                                     non-zero row; a proband that was dragged into the last cut already sits in a slot: its
//                                     occurrences are copy items (source A = its slot, no source B, no one-hot) at the end
//                                     of the last list
//           Emit::None          (rec) the last step is a step like the others; pro_slots lists the slots of the distinct
//                                     probands with a non-zero row for a pass over them after the sweep
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "pedigree_index.h"

namespace genphi {

// One item = one row a launch computes: (destination slot or result row, source slot A, source slot B, first one-hot entry);
// -1 = the zero row.  The one-hot entries of item i are oh_cols[items[i].oh .. items[i + 1].oh) (global column indices,
// ascending); every list of items ends with a sentinel whose .oh closes the last one.  The memory of an int4.
struct alignas(16) SweepItem {
    int32_t dst, a, b, oh;
};

enum class Emit { LeafFirst, EveryProband, None };

struct SweepOptions {
    Emit emit = Emit::LeafFirst;
    bool first_onehot_only = false;   // a duplicated ancestor ID: only its first column gets the one-hot (occ: later rows are zero)
    bool drop_unknown_pro = false;    // proband IDs that are not in the pedigree are ignored instead of a KeyError (rec)
    bool mark_copies = false;         // EveryProband: the copy items of the last list carry source B = -2 instead of -1 (meioses:
                                      // a recursion whose step is not the identity on a single source has to tell them apart)
    bool every_member = false;        // completeness: the columns are generations, not ancestors.  Every member of every cut gets a row
                                      // and a slot (nothing is "none"), no ancestor list and no one-hot columns exist (n_anc = 0 is
                                      // valid, oh_cols stays empty); needs Emit::EveryProband.  n_generations is reported.
};

struct SweepSchedule {
    int64_t n_pro = 0, n_anc = 0;            // as requested (n_pro after drop_unknown_pro)
    std::vector<SweepItem> items;            // every launch's items, each list closed by a sentinel
    std::vector<int32_t> oh_cols;
    std::vector<int64_t> list_begin;         // launch k: items [list_begin[k], list_begin[k + 1] - 1) (the last one a sentinel)
    std::vector<char> list_to_result;
    std::vector<double> list_srcs;           // source rows read, summed over the list's items (algorithmic bytes)
    int64_t peak_slots = 0;
    int32_t n_steps = 0;                     // level steps of the sweep (cuts - 1)
    std::vector<int32_t> pro_slots;          // Emit::None: slots of the distinct probands whose row is not zero
    std::vector<char> anc_is_pro;            // per ancestor column: the ancestor is one of the probands
    int32_t n_generations = 0;               // every_member: 1 + the longest ascent of any listed proband (0 without probands)
};

// Returns 0 or a GENPHI_ERR_* code (include/genphi.h); message in err.  Validates the pedigree (order, duplicates) and the IDs.
int plan_sweep(SweepSchedule &out, int64_t n_ind, const int64_t *ind, const int64_t *father, const int64_t *mother, int64_t n_pro,
               const int64_t *pro_ids, int64_t n_anc, const int64_t *anc_ids, const SweepOptions &opt, std::string &err);

}  // namespace genphi
