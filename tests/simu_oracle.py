"""Two CPU references for gene dropping (gen.simuSample / gen.simuProb; the definition is the text in include/genphi.h) that share
no code with the library, and none with each other beyond the four constants below.

simu_literal   one simulation at a time on Python integers: the whole pedigree, no pruning, no levels, no bit rows.  Its own scalar
               Philox4x32-10 (a block per (ID, side, pair of words), kept in a dict).
SimuVector     numpy over (rows of a level x words): the live set and its levels as the definition states them, one
               vectorised Philox call per level and side, bit rows as uint64.  .plan() alone needs no simulation.
"""
import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85

# (counter, key, output) of Philox4x32-10: the known answers of include/genphi.h
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


# ---------------------------------------------------------------------------------------------------------------- literal
def philox_scalar(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def simu_literal(ind, father, mother, pro, ancestors, states, S, seed):
    """The int8 (len(pro), S) sample, one simulation at a time.  KeyError for an unknown ID."""
    ind = [int(x) for x in ind]
    parents = {x: (int(f), int(m)) for x, f, m in zip(ind, father, mother)}
    fixed = {}
    for a, t in zip(ancestors, states):
        _ = parents[int(a)]
        fixed[int(a)] = int(t)
    # parents before children, whatever the order of the table
    order, placed = [], set()
    todo = list(ind)
    while todo:
        rest = []
        for x in todo:
            if all(q == 0 or q in placed for q in parents[x]):
                order.append(x)
            else:
                rest.append(x)
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

    out = np.zeros((len(pro), S), dtype=np.int8)
    pro = [int(p) for p in pro]
    for p in pro:
        _ = parents[p]
    for s in range(S):
        got = {}                                      # x -> (copy from the father is marked, copy from the mother is marked)
        for x in order:
            if x in fixed:
                got[x] = ((0, 0), (1, 0), (1, 1))[fixed[x]]
                continue
            sides = []
            for side, q in enumerate(parents[x]):
                if q == 0:
                    sides.append(0)
                else:
                    sides.append(got[q][0] if coin(x, side, s) else got[q][1])
            got[x] = tuple(sides)
        for i, p in enumerate(pro):
            out[i, s] = got[p][0] + got[p][1]
    return out


# ------------------------------------------------------------------------------------------------------------- vectorised
def philox_vector(c0, c1, c2, c3, k0, k1):
    """Arrays (or scalars) of 32-bit values -> the four outputs as uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    lo32, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & lo32, (p0 >> sh) ^ c3 ^ k1, p0 & lo32
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & lo32, (k1 + np.uint64(PHILOX_W1)) & lo32
    return c0, c1, c2, c3


class SimuVector:
    def __init__(self, ind, father, mother, pro, ancestors, states):
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
        anc = position(ancestors, False)
        self.state = np.full(n, -1, dtype=np.int64)
        self.state[anc] = np.asarray(states, dtype=np.int64)
        # generation depth: parents first, whatever the order of the table
        depth = np.zeros(n, dtype=np.int64)
        while True:
            d = 1 + np.maximum(np.where(self.fa >= 0, depth[self.fa], -1), np.where(self.mo >= 0, depth[self.mo], -1))
            if np.array_equal(d, depth):
                break
            depth = d
        self.by_depth = np.argsort(depth, kind="stable")
        self._plan()

    def _plan(self):
        n, fa, mo, state = len(self.ind), self.fa.tolist(), self.mo.tolist(), self.state.tolist()
        down, up = [False] * n, [False] * n
        for x in self.by_depth.tolist():
            down[x] = state[x] >= 1 if state[x] >= 0 else any(q >= 0 and down[q] for q in (fa[x], mo[x]))
        for p in self.pro.tolist():
            up[p] = True
        for x in self.by_depth.tolist()[::-1]:
            if up[x]:
                for q in (fa[x], mo[x]):
                    if q >= 0:
                        up[q] = True
        level = [-1] * n
        for x in self.by_depth.tolist():
            if down[x] and up[x]:
                level[x] = 0 if state[x] >= 0 else 1 + max(level[q] if q >= 0 else -1 for q in (fa[x], mo[x]))
        self.level = np.asarray(level, dtype=np.int64)
        self.n_live = int(np.count_nonzero(self.level >= 0))
        self.levels = int(self.level.max()) + 1 if self.n_live else 0
        self.rows_per_level = np.bincount(self.level[self.level >= 0], minlength=self.levels).astype(np.int64)

    def rows(self, S, seed):
        """(P, M): uint64 bit rows (n_ind + 1, words), words a whole number of pairs; the last row is the zero row."""
        n = len(self.ind)
        pairs = (S + 127) // 128
        P = np.zeros((n + 1, 2 * pairs), dtype=np.uint64)
        M = np.zeros((n + 1, 2 * pairs), dtype=np.uint64)
        ones = np.uint64(0xFFFFFFFFFFFFFFFF)
        P[np.flatnonzero((self.level == 0) & (self.state >= 1))] = ones
        M[np.flatnonzero((self.level == 0) & (self.state == 2))] = ones
        ids = self.ind.astype(np.uint64)
        pair = np.arange(pairs, dtype=np.uint64)[None, :]
        for k in range(1, self.levels):
            x = np.flatnonzero(self.level == k)
            idl, idh = (ids[x] & np.uint64(0xFFFFFFFF))[:, None], (ids[x] >> np.uint64(32))[:, None]
            for side, (parent, dst) in enumerate(((self.fa, P), (self.mo, M))):
                q = parent[x]
                live = (q >= 0) & (self.level[np.maximum(q, 0)] >= 0)
                q = np.where(live, q, n)
                o0, o1, o2, o3 = philox_vector(idl, idh, pair, side, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
                T = np.empty((len(x), 2 * pairs), dtype=np.uint64)
                T[:, 0::2] = o0 | (o1 << np.uint64(32))
                T[:, 1::2] = o2 | (o3 << np.uint64(32))
                dst[x] = (T & P[q]) | (~T & M[q])
        return P, M

    def sample(self, S, seed):
        """The int8 (len(pro), S) sample."""
        P, M = self.rows(S, seed)
        rows = np.where(self.level[self.pro] >= 0, self.pro, len(self.ind))

        def bits(A):
            return np.unpackbits(np.ascontiguousarray(A[rows]).astype("<u8").view(np.uint8), axis=1, bitorder="little")[:, :S]

        return (bits(P) + bits(M)).astype(np.int8)


def state_counts(sample):
    """(n_pro, 3) int64: the simulations with 0, 1, 2 copies."""
    return np.stack([(sample == k).sum(axis=1) for k in range(3)], axis=1).astype(np.int64)


def match_counts(sample, state_pro):
    """Per simulation, the probands whose count equals their state: int32 (S,)."""
    return (sample == np.asarray(state_pro).reshape(-1, 1)).sum(axis=0).astype(np.int32)
