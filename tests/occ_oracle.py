"""CPU references for gen.occ (src/describe.jl:184-238) and gen.rec (src/describe.jl:133-145) that share no code with the library
or with each other.

occ_literal / rec_literal   the reference restated: a walk of every ascending path per proband with read-and-reset per ancestor
                            row; a stack search over children per ancestor, filtered by membership in the proband list
occ_exact / rec_exact       Python integers: per proband, path counts pushed from the proband up to its ancestors (children
                            before parents), reduced modulo 2^64 and read as signed only at the end; ancestor sets as
                            arbitrary-precision bit masks pulled down from the founders

All take the pedigree as arrays (ind, father, mother; 0 = unknown parent) in any order and return what the reference returns:
occ a (len(ancestors), len(pro)) int64 matrix ((len(ancestors), 1) for "TOTAL"), rec an int64 vector of len(ancestors).
"""
import numpy as np

M64 = 1 << 64


def _index(ind, father, mother):
    ind = [int(v) for v in ind]
    pos = {v: k for k, v in enumerate(ind)}
    fa = [pos[int(v)] if int(v) != 0 else -1 for v in father]
    mo = [pos[int(v)] if int(v) != 0 else -1 for v in mother]
    return ind, pos, fa, mo


def _signed(v):
    v %= M64
    return v - M64 if v >= (1 << 63) else v


def occ_literal(ind, father, mother, pro, ancestors, typeOcc="IND"):
    ind, pos, fa, mo = _index(ind, father, mother)
    pro_k = [pos[int(p)] for p in pro]                    # KeyError on an unknown ID, as pedigree[ID]
    anc_k = [pos[int(a)] for a in ancestors]
    is_anc = [False] * len(ind)
    for a in anc_k:
        is_anc[a] = True
    occurrence = [0] * len(ind)
    out = np.zeros((len(anc_k), len(pro_k)), dtype=np.int64)
    for j, p in enumerate(pro_k):
        stack = [p]                                       # _occur!: every ascending path, one visit per path
        while stack:
            x = stack.pop()
            if is_anc[x]:
                occurrence[x] += 1
            if fa[x] >= 0:
                stack.append(fa[x])
            if mo[x] >= 0:
                stack.append(mo[x])
        for i, a in enumerate(anc_k):
            out[i, j] = occurrence[a]
            occurrence[a] = 0                             # a duplicated ancestor reads 0 from here on
    if typeOcc == "IND":
        return out
    if typeOcc == "TOTAL":
        return out.sum(axis=1, dtype=np.int64).reshape(-1, 1)
    return None


def rec_literal(ind, father, mother, probandIDs, ancestorIDs):
    ind, pos, fa, mo = _index(ind, father, mother)
    children = [[] for _ in ind]
    for k in range(len(ind)):
        for q in (fa[k], mo[k]):
            if q >= 0:
                children[q].append(k)
    listed = [int(p) for p in probandIDs]                 # only ever the right-hand side of `x in probandIDs`
    coverage = []
    for a in ancestorIDs:
        found = set()
        stack = [pos[int(a)]]                             # KeyError on an unknown ancestor
        while stack:
            x = stack.pop()
            for c in children[x]:
                if c not in found:                        # (the reference pushes again; the set is the same)
                    found.add(c)
                    stack.append(c)
        coverage.append(sum(1 for c in found if ind[c] in listed))
    return np.asarray(coverage, dtype=np.int64)


def _parents_first(fa, mo):
    """Positions in an order with parents before children (Kahn), whatever the order of the arrays."""
    n = len(fa)
    missing = [(fa[k] >= 0) + (mo[k] >= 0) for k in range(n)]
    children = [[] for _ in range(n)]
    for k in range(n):
        for q in (fa[k], mo[k]):
            if q >= 0:
                children[q].append(k)
    order = [k for k in range(n) if missing[k] == 0]
    for x in order:                                       # (the list grows while it is walked)
        for c in children[x]:
            missing[c] -= 1
            if missing[c] == 0:
                order.append(c)
    assert len(order) == n, "cycle in the pedigree"
    return order


class ExactOcc:
    def __init__(self, ind, father, mother):
        self.ind, self.pos, self.fa, self.mo = _index(ind, father, mother)
        self.order = _parents_first(self.fa, self.mo)
        self.when = [0] * len(self.ind)
        for t, x in enumerate(self.order):
            self.when[x] = t

    def paths(self, p):
        """{position: number of ascending paths from position p} as Python integers."""
        fa, mo = self.fa, self.mo
        seen = {p}
        todo = [p]
        while todo:
            x = todo.pop()
            for q in (fa[x], mo[x]):
                if q >= 0 and q not in seen:
                    seen.add(q)
                    todo.append(q)
        w = dict.fromkeys(seen, 0)
        w[p] = 1
        for x in sorted(seen, key=lambda k: self.when[k], reverse=True):      # children before parents
            for q in (fa[x], mo[x]):
                if q >= 0:
                    w[q] += w[x]
        return w


def occ_exact(ind, father, mother, pro, ancestors, typeOcc="IND", sample=None, exact_ints=False):
    """Columns `sample` (indices into pro; all when None).  exact_ints: the unreduced Python integers (object array)."""
    ex = ExactOcc(ind, father, mother)
    pro_k = [ex.pos[int(p)] for p in pro]
    anc_k = [ex.pos[int(a)] for a in ancestors]
    first_row = {}
    for i, a in enumerate(anc_k):
        first_row.setdefault(a, i)                         # only the first row of a duplicated ancestor carries values
    idx = list(range(len(pro_k))) if sample is None else [int(i) for i in sample]
    big = np.zeros((len(anc_k), len(idx)), dtype=object)
    cache = {}
    for c, i in enumerate(idx):
        p = pro_k[i]
        if p not in cache:
            cache[p] = ex.paths(p)
        w = cache[p]
        for a, r in first_row.items():
            big[r, c] = w.get(a, 0)
    if typeOcc == "TOTAL":
        big = big.sum(axis=1).reshape(-1, 1) if len(idx) else np.zeros((len(anc_k), 1), dtype=object)
    elif typeOcc != "IND":
        return None
    if exact_ints:
        return big
    out = np.zeros(big.shape, dtype=np.int64)
    for r in range(big.shape[0]):
        for c in range(big.shape[1]):
            out[r, c] = _signed(int(big[r, c]))
    return out


def rec_exact(ind, father, mother, probandIDs, ancestorIDs):
    ind, pos, fa, mo = _index(ind, father, mother)
    anc_k = [pos[int(a)] for a in ancestorIDs]
    own = [0] * len(ind)
    for j, a in enumerate(anc_k):
        own[a] |= 1 << j
    above = [0] * len(ind)                                 # strict ancestors of each member among the requested ones, a bit per column
    full = [0] * len(ind)                                  # ... and the member itself
    for x in _parents_first(fa, mo):
        m = 0
        for q in (fa[x], mo[x]):
            if q >= 0:
                m |= full[q]
        above[x] = m
        full[x] = m | own[x]
    n_anc = len(anc_k)
    counts = np.zeros(n_anc, dtype=np.int64)
    nbytes = (n_anc + 7) // 8
    for p in {int(p) for p in probandIDs if int(p) in pos}:          # a set; IDs that are not in the pedigree never match
        bits = np.unpackbits(np.frombuffer(above[pos[p]].to_bytes(nbytes, "little"), dtype=np.uint8), bitorder="little")[:n_anc]
        counts += bits
    return counts
