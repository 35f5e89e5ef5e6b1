"""Two CPU references for gen.simuIdentity (the definition is the text in include/genphi.h) that share no code with the library,
and none with each other beyond the Philox constants of tests/simu_oracle.py (its scalar and its numpy Philox are two separate
implementations that already share nothing else).

ident_literal   one simulation at a time on Python integers over the whole pedigree: a label is an integer, an identity state is
                decided on sets of labels.  Its live set is a set walk, its allele table a sorted list.
IdentVector     numpy over (rows of a level x simulations): Int32 labels, the live set and its levels as the definition states
                them, equality tests on labels.  No bit planes: it shares no trick with the library.  The plan (live set, levels,
                allele table, B) alone needs no simulation.
"""
import numpy as np

from simu_oracle import philox_scalar, philox_vector


# ---------------------------------------------------------------------------------------------------------------- literal
def state_of(a, b, c, d):
    """Jacquard's condensed state of the alleles (a, b) of i and (c, d) of j."""
    if a == b and c == d:
        return 1 if a == c else 2
    if a == b:
        return 3 if a in (c, d) else 4
    if c == d:
        return 5 if c in (a, b) else 6
    shared = len({a, b} & {c, d})
    return {2: 7, 1: 8, 0: 9}[shared]


def ident_literal(ind, father, mother, pro, S, seed):
    """(labels int32 (n_pro, 2, S), counts int32 (n_pro, n_pro, 9), alleles [(ID, side)]).  KeyError for an unknown ID."""
    ind = [int(x) for x in ind]
    parents = {x: (int(f), int(m)) for x, f, m in zip(ind, father, mother)}
    pro = [int(p) for p in pro]
    live, todo = set(), list(pro)
    while todo:
        x = todo.pop()
        _ = parents[x]
        if x not in live:
            live.add(x)
            todo.extend(q for q in parents[x] if q)
    alleles = sorted((x, side) for x in live for side in (0, 1) if parents[x][side] == 0)
    label = {a: k for k, a in enumerate(alleles)}
    order, placed = [], set()
    todo = sorted(live)
    while todo:
        rest = []
        for x in todo:
            (order if all(q == 0 or q in placed for q in parents[x]) else rest).append(x)
        placed.update(order[len(placed):])
        assert len(rest) < len(todo), "cycle"
        todo = rest
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    blocks = {}

    def coin(x, side, s):
        w = s // 64
        k = (x, side, w >> 1)
        if k not in blocks:
            xx = x & 0xFFFFFFFFFFFFFFFF
            blocks[k] = philox_scalar((xx & 0xFFFFFFFF, xx >> 32, w >> 1, side), key)
        o = blocks[k]
        word = (o[0] | o[1] << 32) if w % 2 == 0 else (o[2] | o[3] << 32)
        return (word >> (s % 64)) & 1

    n = len(pro)
    labels = np.zeros((n, 2, S), dtype=np.int32)
    counts = np.zeros((n, n, 9), dtype=np.int32)
    for s in range(S):
        got = {}
        for x in order:
            sides = []
            for side, q in enumerate(parents[x]):
                sides.append(label[(x, side)] if q == 0 else got[q][0 if coin(x, side, s) else 1])
            got[x] = tuple(sides)
        for i, p in enumerate(pro):
            labels[i, :, s] = got[p]
            for j, q in enumerate(pro):
                counts[i, j, state_of(*got[p], *got[q]) - 1] += 1
    return labels, counts, alleles


# ------------------------------------------------------------------------------------------------------------- vectorised
class IdentVector:
    def __init__(self, ind, father, mother, pro):
        self.ind = np.asarray(ind, dtype=np.int64)
        n = len(self.ind)
        order = np.argsort(self.ind, kind="stable")
        keys = self.ind[order]

        def position(ids, none_ok):
            ids = np.asarray(ids, dtype=np.int64)
            k = np.clip(np.searchsorted(keys, ids), 0, max(n - 1, 0))
            hit = keys[k] == ids if n else np.zeros(len(ids), bool)
            if none_ok:
                return np.where(hit & (ids != 0), order[k], -1) if n else np.full(len(ids), -1)
            if not np.all(hit):
                raise KeyError(int(ids[np.argmin(hit)]))
            return order[k]

        self.fa, self.mo = position(father, True), position(mother, True)
        self.pro = position(pro, False)
        # level over the whole pedigree (parents first, whatever the order of the table): it depends on the ancestors alone
        level = np.zeros(n, dtype=np.int64)
        while True:
            d = 1 + np.maximum(np.where(self.fa >= 0, level[self.fa], -1), np.where(self.mo >= 0, level[self.mo], -1))
            if np.array_equal(d, level):
                break
            level = d
        live = np.zeros(n, dtype=bool)
        live[self.pro] = True
        for x in np.argsort(level, kind="stable")[::-1].tolist():
            if live[x]:
                for q in (self.fa[x], self.mo[x]):
                    if q >= 0:
                        live[q] = True
        self.live = live
        self.level = np.where(live, level, -1)
        self.n_live = int(live.sum())
        self.levels = int(self.level.max()) + 1
        self.rows_per_level = np.bincount(self.level[live], minlength=self.levels).astype(np.int64)
        # the allele table: ascending by ID, then side
        at = np.flatnonzero(live)
        entries = [(int(self.ind[x]), side, x) for x in at.tolist() for side, par in ((0, self.fa), (1, self.mo)) if par[x] < 0]
        entries.sort()
        self.alleles = np.array([(e[0], e[1]) for e in entries], dtype=np.int64).reshape(-1, 2)
        self._allele_at = np.array([e[2] for e in entries], dtype=np.int64)
        self.n_labels = len(entries)
        self.planes = max(1, int(self.n_labels - 1).bit_length())

    def labels_of_all(self, S, seed):
        """Int32 (n_ind, 2, S): the labels of both sides of everyone (rows outside the live set stay -1)."""
        n = len(self.ind)
        pairs = (S + 127) // 128
        L = np.full((n, 2, S), -1, dtype=np.int32)
        L[self._allele_at, self.alleles[:, 1], :] = np.arange(self.n_labels, dtype=np.int32)[:, None]
        ids = self.ind.astype(np.uint64)
        pair = np.arange(pairs, dtype=np.uint64)[None, :]
        for k in range(1, self.levels):
            x = np.flatnonzero(self.level == k)
            for side, parent in enumerate((self.fa, self.mo)):
                xs = x[parent[x] >= 0]
                if not len(xs):
                    continue
                q = parent[xs]
                idl, idh = (ids[xs] & np.uint64(0xFFFFFFFF))[:, None], (ids[xs] >> np.uint64(32))[:, None]
                o0, o1, o2, o3 = philox_vector(idl, idh, pair, side, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
                T = np.empty((len(xs), 2 * pairs), dtype=np.uint64)
                T[:, 0::2] = o0 | (o1 << np.uint64(32))
                T[:, 1::2] = o2 | (o3 << np.uint64(32))
                bits = np.unpackbits(T.astype("<u8").view(np.uint8), axis=1, bitorder="little")[:, :S].astype(bool)
                L[xs, side, :] = np.where(bits, L[q, 0, :], L[q, 1, :])
        return L

    def labels(self, S, seed):
        """Int32 (n_pro, 2, S)."""
        return np.ascontiguousarray(self.labels_of_all(S, seed)[self.pro])

    def counts(self, S, seed):
        return counts_of(self.labels(S, seed))


def counts_of(labels):
    """Int32 (n_pro, n_pro, 9) from the probands' labels (n_pro, 2, S): equality tests on labels, a row of pairs at a time."""
    n, _, S = labels.shape
    assert labels.min() >= 0
    out = np.zeros((n, n, 9), dtype=np.int32)
    c, d = labels[:, 0, :], labels[:, 1, :]
    cd = c == d
    for i in range(n):
        a, b = labels[i, 0, :][None, :], labels[i, 1, :][None, :]
        ab = np.broadcast_to(a == b, cd.shape)
        ac, ad, bc, bd = a == c, a == d, b == c, b == d
        st = np.full((n, S), 9, dtype=np.int8)
        st[~ab & ~cd & (ac | ad | bc | bd)] = 8
        st[~ab & ~cd & ((ac & bd) | (ad & bc))] = 7
        st[~ab & cd] = 6
        st[~ab & cd & (ac | bc)] = 5
        st[ab & ~cd] = 4
        st[ab & ~cd & (ac | ad)] = 3
        st[ab & cd] = 2
        st[ab & cd & ac] = 1
        for k in range(9):
            out[i, :, k] = (st == k + 1).sum(axis=1)
    return out


def kinship_of(counts, S):
    """(4 c1 + 2 (c3 + c5 + c7) + c8) / (4 S) in Float64."""
    c = counts.astype(np.int64)
    return (4 * c[..., 0] + 2 * (c[..., 2] + c[..., 4] + c[..., 6]) + c[..., 7]) / (4.0 * S)


def swap_roles(counts):
    """counts with the roles of the two individuals exchanged: states 3 <-> 5 and 4 <-> 6, transposed."""
    return np.ascontiguousarray(counts.transpose(1, 0, 2)[..., [0, 1, 4, 5, 2, 3, 6, 7, 8]])
