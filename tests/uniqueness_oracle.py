"""The CPU reference of gen.simuUniqueness (the definition is the text of genphi_unique_* in include/genphi.h): the two tables from
the Int32 labels (n_listed, 2, S) that tests/ident_oracle.py's IdentVector computes for the probands followed by the others.  Per
simulation a np.add.at over (label, simulation) for the distinct members of the population, then per proband a fancy-indexed read-back
of the counts of its two labels and a np.add.at that bins them.  No packed counters, no chunks: it shares no trick with
csrc/unique.hip.  Also the checker of the invariants 1, 7 and 8 of the definition."""
import numpy as np

from ident_oracle import IdentVector


def shares(pop_labels, n_labels):
    """c1 int64 (n_labels, S) from the labels (n_pop, 2, S) of the DISTINCT members of the population: those with at least one side
    equal to the label."""
    n_pop, _, S = pop_labels.shape
    assert pop_labels.min() >= 0 and pop_labels.max() < n_labels
    a, b = pop_labels[:, 0, :], pop_labels[:, 1, :]
    sims = np.broadcast_to(np.arange(S)[None, :], a.shape)
    c1 = np.zeros((n_labels, S), dtype=np.int64)
    np.add.at(c1, (a, sims), 1)
    differ = a != b
    np.add.at(c1, (b[differ], sims[differ]), 1)
    return c1


def tables(pop_labels, n, n_labels, max_share=0):
    """(alleles int32 (n, K), autozygous int32 (n, K)); the first n members of the population are the probands."""
    n_pop, _, S = pop_labels.shape
    K = min(n_pop, max_share) if max_share else n_pop
    c1 = shares(pop_labels, n_labels)
    sims = np.arange(S)
    alleles, autozygous = np.zeros((n, K), dtype=np.int32), np.zeros((n, K), dtype=np.int32)
    for i in range(n):
        a, b = pop_labels[i, 0, :], pop_labels[i, 1, :]
        col_a, col_b = np.minimum(c1[a, sims], K) - 1, np.minimum(c1[b, sims], K) - 1
        assert col_a.min() >= 0 and col_b.min() >= 0                     # the proband itself carries both
        same = a == b
        np.add.at(alleles[i], col_a, 1)
        np.add.at(alleles[i], col_b[~same], 1)
        np.add.at(autozygous[i], col_a[same], 1)
    return alleles, autozygous


class UniqueVector:
    """The reference of one (pedigree, probands, others): labels once at the largest S, cut to the columns a case needs.  ids: the
    distinct probands in ascending row order (the level of the individual, then its position in the pedigree); pop_ids: those
    followed by the distinct others that are not probands."""

    def __init__(self, ind, father, mother, pro, others, S, seed):
        pro, others = np.asarray(pro, dtype=np.int64), np.asarray([] if others is None else others, dtype=np.int64)
        listed = np.concatenate([pro, others])
        self.o = IdentVector(ind, father, mother, listed)
        self.alleles = self.o.alleles
        self.n_labels = self.o.n_labels
        lab = self.o.labels(S, seed)
        _, first = np.unique(listed, return_index=True)                  # one position per distinct ID
        is_pro = np.isin(listed[first], pro)
        at = self.o.pro[first]                                           # positions in the pedigree
        order = np.lexsort((at, self.o.level[at], ~is_pro))              # probands first; then by level, then by position
        self.n = int(is_pro.sum())
        self.n_pop = len(first)
        self.pop_ids = listed[first][order]
        self.ids = self.pop_ids[: self.n]
        self.pop_labels = np.ascontiguousarray(lab[first][order])

    def at(self, S, max_share=0):
        return tables(np.ascontiguousarray(self.pop_labels[:, :, :S]), self.n, self.n_labels, max_share)


def check_rows(alleles, autozygous, S, n_pop):
    """Invariant 1 and the ranges."""
    assert alleles.dtype == autozygous.dtype == np.int32 and alleles.shape == autozygous.shape and 1 <= alleles.shape[1] <= n_pop
    assert alleles.min() >= 0 and autozygous.min() >= 0
    total = alleles.sum(axis=1, dtype=np.int64) + autozygous.sum(axis=1, dtype=np.int64)
    assert np.all(total == 2 * S), total                                                                           # 1
    assert np.all(autozygous.sum(axis=1, dtype=np.int64) <= S)


def check_lumped(full, cut):
    """Invariant 8: a table with fewer columns has the same leading columns, and its last is the sum of the dropped ones."""
    K = cut.shape[1]
    assert full.shape[0] == cut.shape[0] and K <= full.shape[1]
    assert np.array_equal(cut[:, : K - 1], full[:, : K - 1])
    assert np.array_equal(cut[:, K - 1], full[:, K - 1:].sum(axis=1, dtype=np.int64))


def check_founders_and_children(alleles, autozygous, ids, pop_ids, ind, father, mother, S):
    """Invariant 7 on tables of more than one column: a proband that is a founder with no descendant in the population has
    alleles[i, 0] = 2 S; a proband whose parents are both in the population has nothing in column 0.  Returns how many probands of
    either kind there were."""
    assert alleles.shape[1] > 1
    ind, father, mother = (np.asarray(x).tolist() for x in (ind, father, mother))
    parents = dict(zip(ind, zip(father, mother)))
    pop = set(np.asarray(pop_ids).tolist())
    with_descendant = set()                                              # the ancestors of the population, itself apart
    todo = [q for x in pop for q in parents[x] if q]
    while todo:
        x = todo.pop()
        if x not in with_descendant:
            with_descendant.add(x)
            todo.extend(q for q in parents[x] if q)
    lone, children = 0, 0
    for i, x in enumerate(np.asarray(ids).tolist()):
        f, m = parents[x]
        if f == 0 and m == 0 and x not in with_descendant:
            assert alleles[i, 0] == 2 * S and not autozygous[i].any(), (x, alleles[i], autozygous[i])
            lone += 1
        if f and m and f in pop and m in pop:
            assert alleles[i, 0] == 0 and autozygous[i, 0] == 0, (x, alleles[i], autozygous[i])
            children += 1
    return lone, children
