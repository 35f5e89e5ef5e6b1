"""The CPU reference of gen.simuCarriers (the definition is the text of genphi_carry_* in include/genphi.h): the three tables from the
Int32 labels (n_listed, 2, S) that tests/ident_oracle.py's IdentVector computes for the cases followed by the controls.  Per
simulation a np.add.at over (label, simulation) for the distinct cases, a boolean table for the controls, and a second np.add.at
that bins the counts.  No packed counters, no chunks: it shares no trick with csrc/carry.hip."""
import numpy as np

from ident_oracle import IdentVector


def counts(case_labels, n_labels):
    """(c1, c2) int64 (n_labels, S) from the labels (n, 2, S) of the DISTINCT cases: the cases with at least one side / with both
    sides equal to the label."""
    n, _, S = case_labels.shape
    assert n == 0 or (case_labels.min() >= 0 and case_labels.max() < n_labels)
    a, b = case_labels[:, 0, :], case_labels[:, 1, :]
    sims = np.broadcast_to(np.arange(S)[None, :], a.shape)
    c1 = np.zeros((n_labels, S), dtype=np.int64)
    c2 = np.zeros((n_labels, S), dtype=np.int64)
    np.add.at(c1, (a, sims), 1)
    differ = a != b
    np.add.at(c1, (b[differ], sims[differ]), 1)
    np.add.at(c2, (a[~differ], sims[~differ]), 1)
    return c1, c2


def tables(case_labels, control_labels, n_labels, max_count=0):
    """(carriers int32 (n_labels, W), homozygotes int32 (n_labels, W), excluded int32 (n_labels,)) with column 0 left zero, as the
    device delivers them.  The labels are those of the distinct cases and of the distinct controls."""
    n, _, S = case_labels.shape
    W = (min(n, max_count) if max_count else n) + 1
    c1, c2 = counts(case_labels, n_labels)
    x = np.zeros((n_labels, S), dtype=bool)
    if len(control_labels):
        x[control_labels.reshape(-1, S), np.arange(S)[None, :]] = True
    excluded = x.sum(axis=1).astype(np.int32)
    rows = np.broadcast_to(np.arange(n_labels)[:, None], c1.shape)
    out = []
    for c in (c1, c2):
        t = np.zeros((n_labels, W), dtype=np.int32)
        keep = ~x & (c >= 1)
        np.add.at(t, (rows[keep], np.minimum(c[keep], W - 1)), 1)
        out.append(t)
    return out[0], out[1], excluded


def fill(table, excluded, S):
    """The table with column 0 filled as the Python layer fills it: S - excluded - the sum of the columns c >= 1."""
    t = table.copy()
    t[:, 0] = S - excluded.astype(np.int64) - t[:, 1:].sum(axis=1, dtype=np.int64)
    return t


def distinct_positions(ids):
    """The positions of the first occurrence of every distinct ID, in ascending order of the IDs."""
    _, first = np.unique(np.asarray(ids, dtype=np.int64), return_index=True)
    return first


class CarryVector:
    """The reference of one (pedigree, cases, controls): labels once at the largest S, cut to the columns a case needs."""

    def __init__(self, ind, father, mother, cases, controls, S, seed, labels=None):
        cases, controls = np.asarray(cases, dtype=np.int64), np.asarray([] if controls is None else controls, dtype=np.int64)
        self.o = IdentVector(ind, father, mother, np.concatenate([cases, controls]))
        self.alleles = self.o.alleles
        self.n_labels = self.o.n_labels
        lab = self.o.labels(S, seed) if labels is None else labels
        self.case_labels = lab[: len(cases)][distinct_positions(cases)]
        self.control_labels = lab[len(cases):][distinct_positions(controls)] if len(controls) else lab[:0]
        self.n = len(self.case_labels)

    def at(self, S, max_count=0):
        return tables(np.ascontiguousarray(self.case_labels[:, :, :S]), np.ascontiguousarray(self.control_labels[:, :, :S]), self.n_labels, max_count)


def check_invariants(carriers, homozygotes, excluded, alleles, S, cases, controls=()):
    """Invariants 2 - 4 of the definition on the device's tables (column 0 zero or filled: it has weight 0), plus the ranges.  Returns
    the number of founder sides whose carrier is a case."""
    alleles = np.asarray(alleles)
    controls = () if controls is None else controls
    n_labels = len(alleles)
    n = len(np.unique(np.asarray(cases)))
    W = carriers.shape[1]
    assert carriers.dtype == homozygotes.dtype == excluded.dtype == np.int32
    assert carriers.shape == homozygotes.shape == (n_labels, W) and excluded.shape == (n_labels,) and 2 <= W <= n + 1
    assert carriers.min() >= 0 and homozygotes.min() >= 0 and excluded.min() >= 0 and excluded.max() <= S
    weight = np.arange(W, dtype=np.int64)
    wc, wh = carriers.astype(np.int64) @ weight, homozygotes.astype(np.int64) @ weight
    if len(controls) == 0:
        assert not excluded.any()
        if W == n + 1:
            assert int(wc.sum()) + int(wh.sum()) == 2 * n * S                                                       # 2
    assert np.all(wh <= wc)                                                                                         # 3
    some = carriers[:, 1:].sum(axis=1, dtype=np.int64)
    assert np.all(some + excluded <= S) and np.all(homozygotes[:, 1:].sum(axis=1, dtype=np.int64) <= some)
    own = np.isin(alleles[:, 0], np.unique(np.asarray(cases)))
    assert np.all(some[own] == S - excluded[own])                                                                   # 4
    return int(own.sum())
