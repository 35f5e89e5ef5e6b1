"""Two CPU references for gen.gc (src/compute.jl:518-595) that share no code with the library.

gc_literal     the reference restated: children kept in pedigree order (father's list, then mother's), a depth-first walk of
               every path from each ancestor (iterative, in the order _contribute! recurses), 0.5^depth added to a LEAF's
               Float32 accumulator one path at a time, and each proband's accumulator read into its row and reset after every
               ancestor.  One step per path: meant for geneaJi, genea140 (about 0.3 M paths) and small constructed pedigrees.
gc_exact_rows  exact contributions as Python integers scaled by 2^S, one proband at a time: w(p) = 2^S, then every member of
               p's ancestry in reverse rank order hands w(x) / 2 to each of its parents; row p = w at the ancestors.  Cost: the
               size of p's ancestry, so large workloads are checked on a sample of rows.  Rounded once, correctly, to Float32
               (subnormals included), or returned as the integers.
Both keep the reference's rules: only leaves receive contributions, and a proband listed again gets a row of zeros.
"""
import math

import numpy as np


def _index(ind, father, mother):
    ind = [int(x) for x in ind]
    pos = {x: k for k, x in enumerate(ind)}
    fa = [pos[int(x)] if x else -1 for x in father]
    mo = [pos[int(x)] if x else -1 for x in mother]
    return ind, pos, fa, mo


def gc_literal(ind, father, mother, pro, ancestors):
    """The reference's Congen port, path by path, in Float32 (a KeyError for an unknown ID, as the reference's lookup)."""
    ind, pos, fa, mo = _index(ind, father, mother)
    children = [[] for _ in ind]
    for k in range(len(ind)):              # pedigree (rank) order: father's list first, then mother's (src/compute.jl:565-572)
        if fa[k] >= 0:
            children[fa[k]].append(k)
        if mo[k] >= 0:
            children[mo[k]].append(k)
    pro_k = [pos[int(p)] for p in pro]
    anc_k = [pos[int(a)] for a in ancestors]
    contribution = [np.float32(0.0)] * len(ind)
    out = np.zeros((len(pro_k), len(anc_k)), dtype=np.float32)
    for j, a in enumerate(anc_k):
        stack = [(a, 0)]
        while stack:
            x, d = stack.pop()
            if not children[x]:
                # Float32 += Float64 in Julia: the sum in Float64, rounded to Float32 on assignment
                contribution[x] = np.float32(float(contribution[x]) + 0.5 ** d)
            else:
                for c in reversed(children[x]):          # visited in list order
                    stack.append((c, d + 1))
        for i, p in enumerate(pro_k):
            out[i, j] = contribution[p]
            contribution[p] = np.float32(0.0)
    return out


def round_f32(w, S):
    """w / 2^S (w >= 0 an integer) correctly rounded to Float32 (round half to even; subnormals; no overflow: w <= 2^S)."""
    if w == 0:
        return np.float32(0.0)
    E = w.bit_length() - S                   # value in [2^(E-1), 2^E)
    u = max(E - 24, -149)                    # exponent of the Float32 ulp there
    shift = S + u                            # value / 2^u = w / 2^shift
    if shift <= 0:
        q = w << -shift
    else:
        q, r = divmod(w, 1 << shift)
        half = 1 << (shift - 1)
        if r > half or (r == half and q & 1):
            q += 1
    return np.float32(math.ldexp(q, u))


class ExactGC:
    """Exact rows of gen.gc for a pedigree: rows(pro, ancestors, sample) -> Float32 (correctly rounded) or integer rows."""

    def __init__(self, ind, father, mother):
        self.ind, self.pos, self.fa, self.mo = _index(ind, father, mother)
        n = len(self.ind)
        self.has_child = [False] * n
        for k in range(n):
            for q in (self.fa[k], self.mo[k]):
                if q >= 0:
                    self.has_child[q] = True
        # a parents-first order of its own (generation depth, then position) and the longest path
        depth = [0] * n
        order = sorted(range(n), key=lambda k: k)
        changed = True
        while changed:                          # (positions need not be parents-first: iterate to the fixed point)
            changed = False
            for k in order:
                d = 1 + max([depth[q] for q in (self.fa[k], self.mo[k]) if q >= 0], default=-1)
                if d != depth[k]:
                    depth[k], changed = d, True
        self.depth = depth
        self.S = max(depth, default=0) + 1

    def row_int(self, p):
        """{position: w} for leaf proband position p: w = 2^S x contribution of that individual to p."""
        fa, mo, depth = self.fa, self.mo, self.depth
        seen = {p}
        todo = [p]
        while todo:
            x = todo.pop()
            for q in (fa[x], mo[x]):
                if q >= 0 and q not in seen:
                    seen.add(q)
                    todo.append(q)
        w = dict.fromkeys(seen, 0)
        w[p] = 1 << self.S
        for x in sorted(seen, key=lambda k: depth[k], reverse=True):     # children before parents
            v = w[x]
            if v == 0:
                continue
            for q in (fa[x], mo[x]):
                if q >= 0:
                    assert v % 2 == 0, "inexact halving"
                    w[q] += v // 2
        return w

    def rows(self, pro, ancestors, sample=None, exact_ints=False):
        """Rows `sample` (indices into pro; all when None) of gen.gc(pro, ancestors).  Float32, or integers / 2^S."""
        pro_k = [self.pos[int(p)] for p in pro]
        anc_k = [self.pos[int(a)] for a in ancestors]
        first = {}
        for i, p in enumerate(pro_k):
            first.setdefault(p, i)
        idx = range(len(pro_k)) if sample is None else list(sample)
        out = (np.zeros((len(idx), len(anc_k)), dtype=object) if exact_ints else np.zeros((len(idx), len(anc_k)), dtype=np.float32))
        for r, i in enumerate(idx):
            p = pro_k[i]
            if first[p] != i or self.has_child[p]:
                continue                             # repeated or non-leaf proband: zeros
            w = self.row_int(p)
            for j, a in enumerate(anc_k):
                v = w.get(a, 0)
                out[r, j] = v if exact_ints else round_f32(v, self.S)
        return out


def gc_exact_rows(ind, father, mother, pro, ancestors, sample=None):
    """Correctly rounded Float32 rows of gen.gc (see ExactGC)."""
    return ExactGC(ind, father, mother).rows(pro, ancestors, sample)


def divergence_pedigree(n_ladder=8, chain=21):
    """A pedigree where the reference's path-by-path Float32 sums differ from the correctly rounded contribution.

    Ancestor 1 (a founder) has an elder child E, listed first, so the depth-first walk takes the path 1 -> E -> P of
    length 2 first: P's accumulator holds 0.25.  Then 2^(n_ladder - 1) paths of length n_ladder + chain + 1 run from 1 down
    a ladder (U_k, V_k both children of U_{k-1} and V_{k-1}) and a chain of `chain` single descendants to P.  With the
    defaults 128 paths of length 30 each add 2^-30, less than half an ulp of 0.25 (2^-26): the reference keeps 0.25; the
    exact value is 0.25 + 2^-23, a Float32.  Returns (ind, father, mother, sex, proband, ancestor)."""
    ind, fa, mo = [], [], []

    def add(f, m):
        ind.append(len(ind) + 1)
        fa.append(f)
        mo.append(m)
        return ind[-1]

    A = add(0, 0)
    F = add(0, 0)                                    # A's mate
    E = add(A, F)                                    # the elder child: listed before the ladder
    u, v = add(A, F), add(A, F)
    for _ in range(n_ladder - 1):
        m1, m2 = add(0, 0), add(0, 0)
        del m1, m2                                   # (founders between levels keep the IDs of a level together)
        u, v = add(u, v), add(u, v)
    z = u
    for _ in range(chain):
        mate = add(0, 0)
        z = add(z, mate)
    P = add(E, z)
    a = lambda x: np.asarray(x, dtype=np.int64)
    sex = np.ones(len(ind), dtype=np.int64)
    return a(ind), a(fa), a(mo), sex, P, A
