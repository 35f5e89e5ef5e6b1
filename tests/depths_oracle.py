"""CPU oracles for gen.depths: over all ascending paths from a proband to an ancestor, their number, the shortest, the longest and
the mean length.  Pure Python on dictionaries and Python integers; shares no code with the library.

depths_literal  reduces the reference's own _findDistance lists (src/describe.jl:241-279): _get_paths builds every ascending path as a
                list of IDs (get_paths_literal of tests/mrca_oracle.py), the paths that start at the ancestor are its list, and the four
                statistics are len, min, max and sum / len of it.  Exponential in the depth: small inputs only.
depths_exact    ascends level by level with a counter of individuals per proband: level k holds, per individual, the number of paths
                of exactly k meioses that reach it.  Linear in the size of the ancestry times its depth: any input.
Both return a Depths of arrays (min, max int16 with -1 = no path; paths int64; mean float64 with NaN = no path) of shape
(len(pro), len(anc)), and keep the exact sums of the lengths (Python integers) for the reductions:
reduce_depths(d, "proband")  over the ancestors of each row, reduce_depths(d, "ancestor") over the probands of each column; their mean
is float(sum of the sums) / float(sum of the counts).  Both oracles must agree wherever both can run (tests/test_depth_host.py)."""
from collections import Counter

import numpy as np

from mrca_oracle import _parents, get_paths_literal


class Depths:
    def __init__(self, P, S, lo, hi):
        """P, S: nested lists of Python integers (counts, sums of lengths); lo, hi: nested lists, -1 = no path."""
        self.P, self.S = P, S
        self.min = np.array(lo, dtype=np.int16)
        self.max = np.array(hi, dtype=np.int16)
        self.paths = np.array(P, dtype=np.int64)
        flatP = np.array(P, dtype=object).ravel()
        flatS = np.array(S, dtype=object).ravel()
        self.mean = np.array([float(s) / float(p) if p else np.nan for p, s in zip(flatP, flatS)], dtype=np.float64).reshape(self.paths.shape)


def _table(per_proband, pro, anc):
    """per_proband(ID) -> {ancestor: (P, S, min, max)}; one row per listed proband, one column per listed ancestor."""
    cache = {}
    P, S, lo, hi = [], [], [], []
    for ID in pro:
        ID = int(ID)
        if ID not in cache:
            cache[ID] = per_proband(ID)
        row = [cache[ID].get(int(a), (0, 0, -1, -1)) for a in anc]
        P.append([r[0] for r in row])
        S.append([r[1] for r in row])
        lo.append([r[2] for r in row])
        hi.append([r[3] for r in row])
    d = Depths(P, S, lo, hi)
    for name in ("min", "max", "paths", "mean"):
        setattr(d, name, getattr(d, name).reshape(len(pro), len(anc)))
    return d


def _check_ids(par, pro, anc):
    for i in list(pro) + list(anc):
        par[int(i)]                                      # KeyError on an unknown ID


def depths_literal(ind, father, mother, pro, anc):
    par = _parents(ind, father, mother)
    _check_ids(par, pro, anc)

    def per_proband(ID):
        lengths = {}
        for path in get_paths_literal(par, ID):          # _findDistance: the paths that start at the ancestor, their lengths
            lengths.setdefault(path[0], []).append(len(path) - 1)
        return {a: (len(v), sum(v), min(v), max(v)) for a, v in lengths.items()}

    return _table(per_proband, pro, anc)


def depths_exact(ind, father, mother, pro, anc):
    par = _parents(ind, father, mother)
    _check_ids(par, pro, anc)

    def per_proband(ID):
        found = {}
        level, k = Counter({ID: 1}), 0
        while level:
            nxt = Counter()
            for x, c in level.items():
                if x in found:
                    P, S, lo, _ = found[x]
                    found[x] = (P + c, S + c * k, lo, k)
                else:
                    found[x] = (c, c * k, k, k)
                for p in par[x]:
                    if p:
                        nxt[p] += c
            level, k = nxt, k + 1
        return found

    return _table(per_proband, pro, anc)


def reduce_depths(d, by):
    """The four vectors of a Depths reduced over its columns (by = "proband") or its rows (by = "ancestor")."""
    n_pro, n_anc = d.paths.shape
    lines = [[(i, j) for j in range(n_anc)] for i in range(n_pro)] if by == "proband" else [[(i, j) for i in range(n_pro)] for j in range(n_anc)]
    P, S, lo, hi = [], [], [], []
    for line in lines:
        hit = [(i, j) for i, j in line if d.P[i][j]]
        P.append(sum(d.P[i][j] for i, j in hit))
        S.append(sum(d.S[i][j] for i, j in hit))
        lo.append(min((int(d.min[i, j]) for i, j in hit), default=-1))
        hi.append(max((int(d.max[i, j]) for i, j in hit), default=-1))
    return Depths(P, S, lo, hi)
