"""The CPU reference of gen.simuOrigins (the definition is the text of genphi_origin_* in include/genphi.h): the four tables from the
Int32 labels (n_listed, 2, S) that tests/ident_oracle.py's IdentVector computes for the list as given.  A loop over the simulations
with one np.bincount per group: no packed counters, no chunks, it shares no trick with csrc/origin.hip.  Also here: the count of
matching copy pairs proband by proband (the definition of m_aa and m_ab taken literally), the exact expected allele frequencies and
kinships by host recursions, and check_invariants for the invariants 1, 4, 5, 6 and 7 of the definition."""
import numpy as np

from ident_oracle import IdentVector


def pair_index(a, b, G):
    """The position of the pair a <= b in the upper triangle, row-major."""
    return a * G - a * (a - 1) // 2 + (b - a)


def tables(labels, group, G, n_labels):
    """(copies int64 (G, L), autozygous int64 (G, L), matches int64 (P, L), autozygous_pro int32 (n, L)) from the labels (n, 2, S) of
    the DISTINCT grouped probands and their groups (n,) in 0 .. G - 1."""
    n, _, S = labels.shape
    assert n == 0 or (labels.min() >= 0 and labels.max() < n_labels)
    group = np.asarray(group)
    P = G * (G + 1) // 2
    copies, autozygous = np.zeros((G, n_labels), dtype=np.int64), np.zeros((G, n_labels), dtype=np.int64)
    matches = np.zeros((P, n_labels), dtype=np.int64)
    by_pro = np.zeros((n, n_labels), dtype=np.int32)
    members = [np.flatnonzero(group == a) for a in range(G)]
    both = labels[:, 0, :] == labels[:, 1, :]
    rows, sims = np.nonzero(both)
    np.add.at(by_pro, (rows, labels[rows, 0, sims]), 1)
    filled = [a for a in range(G) if len(members[a])]
    first = np.array([pair_index(a, a, G) for a in range(G)])
    for s in range(S):
        k = np.zeros((G, n_labels), dtype=np.int64)
        for a in filled:
            m = members[a]
            k[a] = np.bincount(labels[m, :, s].ravel(), minlength=n_labels)                      # a side is a gene copy
            c2 = np.bincount(labels[m, 0, s][both[m, s]], minlength=n_labels)
            c1 = k[a] - c2
            copies[a] += k[a]
            autozygous[a] += c2
            matches[first[a]] += (k[a] * k[a] - c1 - 3 * c2) // 2
        for a in filled[:-1]:
            at = np.flatnonzero(k[a])                                                            # k_a k_b is 0 elsewhere
            matches[first[a] + 1:first[a] + G - a, at] += k[a, at] * k[a + 1:, at]               # the pairs (a, a + 1 .. G - 1)
    return copies, autozygous, matches, by_pro


def matches_by_pairs(labels, group, G, n_labels):
    """matches (P, L) with the definition taken literally: every pair of different probands, every one of its four pairs of sides."""
    n, _, S = labels.shape
    out = np.zeros((G * (G + 1) // 2, n_labels), dtype=np.int64)
    for i in range(n):
        for j in range(i + 1, n):
            a, b = sorted((int(group[i]), int(group[j])))
            for x in (0, 1):
                for y in (0, 1):
                    same = labels[i, x] == labels[j, y]
                    np.add.at(out[pair_index(a, b, G)], labels[i, x][same], 1)
    return out


def distinct_grouped(ids, groups):
    """The positions in the list of the first occurrence of every distinct ID with a group >= 0, in order of first appearance."""
    ids = np.asarray(ids, dtype=np.int64)
    at = np.arange(len(ids)) if groups is None else np.flatnonzero(np.asarray(groups) >= 0)
    _, first = np.unique(ids[at], return_index=True)
    return at[np.sort(first)]


class OriginVector:
    """The reference of one (pedigree, list, groups): labels once at the largest S, cut to the columns a case needs."""

    def __init__(self, ind, father, mother, pro, groups, G, S, seed):
        pro = np.asarray(pro, dtype=np.int64)
        self.o = IdentVector(ind, father, mother, pro)
        self.alleles, self.n_labels, self.G = self.o.alleles, self.o.n_labels, G
        at = distinct_grouped(pro, groups)
        self.pro = pro[at]
        self.group = np.zeros(len(at), dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)[at]
        self.sizes = np.bincount(self.group, minlength=G).astype(np.int64)
        self.labels = np.ascontiguousarray(self.o.labels(S, seed)[at])
        self.n = len(at)
        self._cache = {}

    def at(self, S):
        if S not in self._cache:
            self._cache[S] = tables(np.ascontiguousarray(self.labels[:, :, :S]), self.group, self.G, self.n_labels)
        return self._cache[S]


def expected_frequency(o, pro, group, G):
    """(G, n_labels) Float64: the exact expected frequency of every founder allele among the gene copies of every group, by the
    recursion of gene contributions over the IdentVector o: a founder side carries its own label, any other side one of the parent's
    two with probability 1/2 each."""
    n = len(o.ind)
    side = np.zeros((n, 2, o.n_labels))
    side[o._allele_at, o.alleles[:, 1], np.arange(o.n_labels)] = 1.0
    for x in np.argsort(o.level, kind="stable").tolist():
        if o.level[x] < 0:
            continue
        for s, parent in enumerate((o.fa, o.mo)):
            if parent[x] >= 0:
                side[x, s] = 0.5 * (side[parent[x], 0] + side[parent[x], 1])
    where = {int(i): k for k, i in enumerate(o.ind.tolist())}
    out = np.zeros((G, o.n_labels))
    sizes = np.bincount(group, minlength=G)
    for p, a in zip(pro.tolist(), np.asarray(group).tolist()):
        out[a] += 0.5 * (side[where[p], 0] + side[where[p], 1]) / sizes[a]
    return out


def exact_kinship(o, pro, group, G):
    """(G, G) Float64: the exact mean kinship within (pairs of different probands) and between groups, by the tabular recursion over
    the whole pedigree of the IdentVector o; NaN where there is no pair."""
    n = len(o.ind)
    level = np.zeros(n, dtype=np.int64)
    while True:
        d = 1 + np.maximum(np.where(o.fa >= 0, level[o.fa], -1), np.where(o.mo >= 0, level[o.mo], -1))
        if np.array_equal(d, level):
            break
        level = d
    phi = np.zeros((n, n))
    done = []
    for x in np.argsort(level, kind="stable").tolist():
        f, m = int(o.fa[x]), int(o.mo[x])
        for y in done:
            phi[x, y] = phi[y, x] = 0.5 * ((phi[f, y] if f >= 0 else 0.0) + (phi[m, y] if m >= 0 else 0.0))
        phi[x, x] = 0.5 * (1.0 + (phi[f, m] if f >= 0 and m >= 0 else 0.0))
        done.append(x)
    where = {int(i): k for k, i in enumerate(o.ind.tolist())}
    at = np.array([where[p] for p in pro.tolist()])
    out = np.full((G, G), np.nan)
    group = np.asarray(group)
    for a in range(G):
        for b in range(a, G):
            ia, ib = at[group == a], at[group == b]
            block = phi[np.ix_(ia, ib)]
            if a == b and len(ia) >= 2:
                out[a, a] = (block.sum() - np.trace(block)) / (len(ia) * (len(ia) - 1))
            elif a != b and len(ia) and len(ib):
                out[a, b] = out[b, a] = block.mean()
    return out


def merge(copies, autozygous, matches, G, parts):
    """The tables of the grouping whose group A is the union of the groups parts[A] (invariant 4)."""
    H = len(parts)
    c = np.stack([copies[p].sum(axis=0) for p in parts])
    z = np.stack([autozygous[p].sum(axis=0) for p in parts])
    m = np.zeros((H * (H + 1) // 2, copies.shape[1]), dtype=np.int64)
    for A in range(H):
        for B in range(A, H):
            for a in parts[A]:
                for b in parts[B]:
                    if A != B or a <= b:
                        m[pair_index(A, B, H)] += matches[pair_index(min(a, b), max(a, b), G)]
    return c, z, m


def check_invariants(copies, autozygous, matches, by_pro, sizes, S, alleles=None, pro=None, group=None, merged=None, other=None):
    """Invariants 1, 4, 5, 6 and 7 of the definition on one set of tables, plus the shapes and the ranges.  merged: the (copies,
    autozygous, matches) of the same list in ONE group (4).  by_pro, with group: the rows follow pro (5); with alleles too: the listed
    founders (6).  other: tables that must hold the same bytes (7).  Returns the number of listed founders seen."""
    sizes = np.asarray(sizes, dtype=np.int64)
    G, L = copies.shape
    P = G * (G + 1) // 2
    assert copies.dtype == autozygous.dtype == matches.dtype == np.int64
    assert autozygous.shape == (G, L) and matches.shape == (P, L) and len(sizes) == G
    assert copies.min() >= 0 and autozygous.min() >= 0 and matches.min() >= 0 and np.all(2 * autozygous <= copies)
    assert np.array_equal(copies.sum(axis=1), 2 * sizes * S)                                                        # 1
    for a in range(G):
        for b in range(a, G):
            pairs = sizes[a] * (sizes[a] - 1) // 2 if a == b else sizes[a] * sizes[b]
            assert matches[pair_index(a, b, G)].sum() <= 4 * pairs * S
    if merged is not None:                                                                                          # 4
        for got, want in zip(merge(copies, autozygous, matches, G, [list(range(G))]), merged):
            assert np.array_equal(got, want)
    founders = 0
    if by_pro is not None:
        assert by_pro.dtype == np.int32 and by_pro.shape == (int(sizes.sum()), L) and by_pro.min() >= 0 and by_pro.max(initial=0) <= S
        if group is not None:                                                                                       # 5
            group = np.asarray(group)
            for a in range(G):
                assert np.array_equal(by_pro[group == a].sum(axis=0, dtype=np.int64), autozygous[a])
    if alleles is not None and pro is not None and group is not None:                                               # 6
        alleles, group = np.asarray(alleles), np.asarray(group)
        for i, p in enumerate(np.asarray(pro).tolist()):
            own = np.flatnonzero(alleles[:, 0] == p)
            if len(own) != 2:
                continue                                                                                            # not a founder with both parents unknown
            founders += 1
            assert np.all(copies[group[i], own] >= S)
            if by_pro is not None:
                assert not by_pro[i].any()
            if sizes[group[i]] == 1:
                assert np.all(copies[group[i], own] == S) and not autozygous[group[i]].any()
                for j, q in enumerate(np.asarray(pro).tolist()):
                    if j != i and sizes[group[j]] == 1 and np.sum(alleles[:, 0] == q) == 2:
                        a, b = sorted((int(group[i]), int(group[j])))
                        assert not matches[pair_index(a, b, G)].any()
    if other is not None:                                                                                           # 7
        for got, want in zip((copies, autozygous, matches, by_pro), other):
            if got is not None and want is not None:
                assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
    return founders
