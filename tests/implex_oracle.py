"""CPU references for gen.implex (GENLIB's gen.implex; the definition is in include/genphi.h): two implementations that share no
code with the library and none with each other beyond the parent lookup.

  implex_literal    per proband, Python sets, generation by generation: A_0 = {p}, A_{g+1} = the known parents of A_g
  implex_frontier   one pass for all probands: a Python integer per individual holds the probands as bits, over the union
                    frontier U_g (the individuals at exactly g meioses from any listed proband); also returns |U_g|

Both return (counts, rows): counts an int64 (n_pro, G) array, G = 1 + the longest ascent of any listed proband; rows the
list of |U_g| (implex_literal builds it as the union of its per-proband sets)."""
from fractions import Fraction

import numpy as np


def _parents(ind, father, mother):
    par = {}
    for i, f, m in zip(np.asarray(ind).tolist(), np.asarray(father).tolist(), np.asarray(mother).tolist()):
        par[i] = tuple(sorted({p for p in (f, m) if p != 0}))
    return par


def implex_literal(ind, father, mother, pro, only_new=False):
    par = _parents(ind, father, mother)
    per_pro, unions = [], []
    for p in np.asarray(pro).tolist():
        if p not in par:
            raise KeyError(p)
        cur, seen, sizes, g = {p}, set(), [], 0
        while cur:
            if len(unions) <= g:
                unions.append(set())
            unions[g] |= cur
            sizes.append(len(cur - seen) if only_new else len(cur))
            seen |= cur
            cur = {q for x in cur for q in par[x]}
            g += 1
        per_pro.append(sizes)
    G = max(len(s) for s in per_pro)
    counts = np.zeros((len(per_pro), G), dtype=np.int64)
    for i, s in enumerate(per_pro):
        counts[i, :len(s)] = s
    return counts, [len(u) for u in unions]


def implex_frontier(ind, father, mother, pro, only_new=False):
    par = _parents(ind, father, mother)
    pro = np.asarray(pro).tolist()
    bits = {}
    for i, p in enumerate(pro):
        if p not in par:
            raise KeyError(p)
        bits[p] = bits.get(p, 0) | (1 << i)
    seen = {}
    columns, rows = [], []
    while bits:
        rows.append(len(bits))
        if only_new:
            for x in bits:
                old = seen.get(x, 0)
                seen[x] = old | bits[x]
                bits[x] &= ~old
        col = [0] * len(pro)
        for b in bits.values():
            while b:
                low = b & -b
                col[low.bit_length() - 1] += 1
                b ^= low
        columns.append(col)
        nxt = {}
        for x, b in bits.items():
            for q in par[x]:
                nxt[q] = nxt.get(q, 0) | b
        bits = nxt
    return np.array(columns, dtype=np.int64).T.copy().reshape(len(pro), len(columns)), rows


def ind_matrix(counts):
    """ "IND": (G, n_pro) float64, count / 2^g * 100 in that order."""
    G = counts.shape[1]
    return np.ascontiguousarray((counts.astype(np.float64) / np.ldexp(1.0, np.arange(G)) * 100.0).T)


def mean_column(counts):
    """ "MEAN": (G, 1) float64, the exact rational mean of the percentages rounded once."""
    n, G = counts.shape
    return np.array([[float(Fraction(100 * sum(int(v) for v in counts[:, g]), (1 << g) * n))] for g in range(G)])
