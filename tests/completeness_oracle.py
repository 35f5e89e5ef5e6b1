"""CPU references for gen.completeness (src/describe.jl:73-125) and gen.depth (src/describe.jl:43-66) that share no code with the
library or with each other.

completeness_literal   the reference restated: a walk of every ascending path per proband that fills a Python list per proband
                       (grown by one entry the first time a generation is reached), entry = count / 2^g * 100, the row of 100s
                       on top, genNo selection, and for "MEAN" the sequential Float64 sum over the probands divided by their
                       number.  Exponential in the depth: for small pedigrees.
completeness_exact     Python integers: P[x][g] = P[father][g - 1] + P[mother][g - 1], P[x][0] = 1, memoised per individual
                       (parents before children); returns the (len(pro), G) counts and the (G, len(pro)) "IND" matrix
mean_fraction          the exact rational mean per generation from the counts (fractions.Fraction)
depth_literal          _max_depth without memory for every individual, and the maximum
depth_exact            memoised depths (parents before children), and the maximum

All take the pedigree as arrays (ind, father, mother; 0 = unknown parent) in any order.
"""
from fractions import Fraction

import numpy as np


def _index(ind, father, mother):
    ind = [int(v) for v in ind]
    pos = {v: k for k, v in enumerate(ind)}
    fa = [pos[int(v)] if int(v) != 0 else -1 for v in father]
    mo = [pos[int(v)] if int(v) != 0 else -1 for v in mother]
    return ind, pos, fa, mo


def _walk(fa, mo, p):
    """_completeness!(Int[], proband, 0): one visit per ascending path."""
    comp = []
    stack = [(p, 0)]
    while stack:
        x, d = stack.pop()
        if (fa[x] >= 0 or mo[x] >= 0) and len(comp) < d + 1:
            comp.append(0)
        for parent in (fa[x], mo[x]):
            if parent >= 0:
                comp[d] += 1
                stack.append((parent, d + 1))
    return comp


def completeness_literal(ind, father, mother, pro, genNo=None, type="MEAN"):
    ind, pos, fa, mo = _index(ind, father, mother)
    pro_k = [pos[int(p)] for p in pro]                    # KeyError on an unknown ID, as pedigree[ID]
    comps = [_walk(fa, mo, p) for p in pro_k]
    max_depth = max(len(c) for c in comps)                # ValueError on an empty list, as maximum of an empty collection
    matrix = np.zeros((max_depth + 1, len(pro_k)), dtype=np.float64)
    matrix[0, :] = 100.0
    for column, comp in enumerate(comps):
        for row, count in enumerate(comp, start=1):
            matrix[row, column] = float(count) / float(2 ** row) * 100.0
    if genNo is not None and len(genNo):
        if any(g < 0 or g >= matrix.shape[0] for g in genNo):
            raise IndexError("generation out of range")   # BoundsError
        matrix = matrix[[int(g) for g in genNo], :]
    if type == "IND":
        return matrix
    if type == "MEAN":
        out = np.zeros((matrix.shape[0], 1), dtype=np.float64)
        for r in range(matrix.shape[0]):
            acc = 0.0
            for c in range(matrix.shape[1]):              # sum(matrix, dims=2): one row, left to right
                acc += float(matrix[r, c])
            out[r, 0] = acc / len(pro_k)
        return out
    return None


def _paths(fa, mo, targets):
    """P[x] = [1, P[fa][0] + P[mo][0], ...] as Python ints for every individual the targets ascend to."""
    memo = {}
    for t in targets:
        stack = [t]
        while stack:
            x = stack[-1]
            if x in memo:
                stack.pop()
                continue
            waiting = [q for q in (fa[x], mo[x]) if q >= 0 and q not in memo]
            if waiting:
                stack.extend(waiting)
                continue
            rows = [memo[q] for q in (fa[x], mo[x]) if q >= 0]
            up = [sum(r[g] for r in rows if g < len(r)) for g in range(max((len(r) for r in rows), default=0))]
            memo[x] = [1] + up
            stack.pop()
    return memo


def completeness_exact(ind, father, mother, pro):
    """(counts, matrix): counts int64 (len(pro), G) (object dtype where a count needs more than 63 bits), matrix float64 (G, len(pro))."""
    ind, pos, fa, mo = _index(ind, father, mother)
    pro_k = [pos[int(p)] for p in pro]
    memo = _paths(fa, mo, pro_k)
    G = max(len(memo[p]) for p in pro_k)
    rows = [memo[p] + [0] * (G - len(memo[p])) for p in pro_k]
    big = any(v >= 1 << 63 for r in rows for v in r)
    counts = np.array(rows, dtype=object if big else np.int64).reshape(len(pro_k), G)
    matrix = np.zeros((G, len(pro_k)), dtype=np.float64)
    for i, r in enumerate(rows):
        for g, v in enumerate(r):
            matrix[g, i] = float(v) / float(2 ** g) * 100.0
    return counts, matrix


def mean_fraction(counts):
    """Per generation, the exact mean of count / 2^g * 100 over the rows of counts."""
    n, G = counts.shape
    return [Fraction(sum(int(counts[i, g]) for i in range(n)) * 100, (2 ** g) * n) for g in range(G)]


def depth_literal(ind, father, mother):
    ind, pos, fa, mo = _index(ind, father, mother)

    def max_depth(x):
        fd = md = 1
        if fa[x] >= 0:
            fd += max_depth(fa[x])
        if mo[x] >= 0:
            md += max_depth(mo[x])
        return max(fd, md)

    out = 0
    for x in range(len(ind)):
        out = max(out, max_depth(x))
    return out


def depth_exact(ind, father, mother, leaves_only=False):
    ind, pos, fa, mo = _index(ind, father, mother)
    memo = _paths(fa, mo, range(len(ind)))
    has_child = [False] * len(ind)
    for q in fa + mo:
        if q >= 0:
            has_child[q] = True
    return max((len(memo[x]) for x in range(len(ind)) if not (leaves_only and has_child[x])), default=0)
