"""The CPU reference of gen.simuRetention (the definition is the text of genphi_retain_* in include/genphi.h): the reductions of
the probands' Int32 labels (n_pro, 2, S) that tests/ident_oracle.py's IdentVector computes.  A boolean presence table
(n_labels, S) filled by fancy indexing, its sums along each axis, and `both` from the IDs of the allele table.  No bitmaps, no
chunks: it shares no trick with csrc/retain.hip."""
import numpy as np

from ident_oracle import IdentVector


def presence(labels, n_labels):
    """bool (n_labels, S): some listed proband carries the label on either side in the simulation."""
    n, _, S = labels.shape
    assert labels.min() >= 0 and labels.max() < n_labels
    table = np.zeros((n_labels, S), dtype=bool)
    table[labels.reshape(2 * n, S), np.arange(S)[None, :]] = True
    return table


def reductions(labels, alleles):
    """(survived int32 (n_labels,), both int32 (n_labels,), distinct int32 (S,)) from the labels and the allele table (n_labels, 2)."""
    alleles = np.asarray(alleles)
    n_labels = len(alleles)
    table = presence(labels, n_labels)
    survived = table.sum(axis=1).astype(np.int32)
    distinct = table.sum(axis=0).astype(np.int32)
    both = np.zeros(n_labels, dtype=np.int32)
    pair = np.flatnonzero(alleles[:-1, 0] == alleles[1:, 0])                    # l and l + 1 belong to one ID: l is its side 0
    both[pair] = (table[pair] & table[pair + 1]).sum(axis=1)
    return survived, both, distinct


class RetainVector:
    """The reference of one (pedigree, proband list): labels once at the largest S, cut to the columns a case needs."""

    def __init__(self, ind, father, mother, pro, S, seed):
        self.o = IdentVector(ind, father, mother, pro)
        self.alleles = self.o.alleles
        self.labels = self.o.labels(S, seed)

    def at(self, S):
        return reductions(np.ascontiguousarray(self.labels[:, :, :S]), self.alleles)


def check_invariants(survived, both, distinct, alleles, S, listed):
    """Invariants 1-4 of the definition, on any three arrays."""
    alleles = np.asarray(alleles)
    n_labels = len(alleles)
    listed = np.unique(np.asarray(listed))
    assert survived.dtype == both.dtype == distinct.dtype == np.int32
    assert survived.shape == both.shape == (n_labels,) and distinct.shape == (S,)
    assert int(distinct.sum(dtype=np.int64)) == int(survived.sum(dtype=np.int64))                                   # 1
    assert distinct.min() >= 1 and distinct.max() <= min(n_labels, 2 * len(listed))                                # 2
    pair = np.zeros(n_labels, dtype=bool)
    pair[:-1] = alleles[:-1, 0] == alleles[1:, 0]
    assert np.all(both[~pair] == 0)
    at = np.flatnonzero(pair)
    assert np.all(both[at] <= np.minimum(survived[at], survived[at + 1]))                                           # 3
    assert np.all(survived[at].astype(np.int64) + survived[at + 1] - both[at] <= S)
    assert survived.min() >= 0 and survived.max() <= S and both.min() >= 0
    own = np.isin(alleles[:, 0], listed)
    assert np.all(survived[own] == S)                                                                               # 4
    return int(own.sum())
