"""The CPU reference of gen.simuSharing (the definition is the text in include/genphi.h, genphi_link_*).  It shares no code with
the library: the plan (live set, levels, allele table) is that of tests/ident_oracle.py, the Philox block is the numpy one of
tests/simu_oracle.py, and everything else is stated on single loci: no bit planes and no prefix tricks.

crossover_words  X by the fold of the definition, all sixteen words of it, nothing skipped
transmission     T as np.cumsum(bits) & 1 over the unpacked bits of X
LinkVector       Int32 labels (rows x sides x simulations x loci), copied from the parents locus by locus under T
sums_of          the six sums of every pair from labels, by comparison; runs counted with np.diff
"""
import numpy as np

from ident_oracle import IdentVector
from simu_oracle import philox_vector

SH = np.uint64(32)


def _block(idl, idh, s, side, w, d, seed):
    """(w0, w1) of block d for arrays of IDs (split), simulations and words."""
    c3 = np.uint64(0x80000000) | np.uint64(side) | (np.asarray(w, dtype=np.uint64) << np.uint64(1)) | np.uint64(d << 8)
    o0, o1, o2, o3 = philox_vector(idl, idh, s, c3, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return o0 | (o1 << SH), o2 | (o3 << SH)


def crossover_words(ids, side, sims, W, q, seed):
    """uint64 (len(ids), len(sims), W): X(w) of every (ID, simulation) for one side."""
    ids = np.asarray(ids, dtype=np.int64).astype(np.uint64)
    idl, idh = (ids & np.uint64(0xFFFFFFFF))[:, None, None], (ids >> SH)[:, None, None]
    s = np.asarray(sims, dtype=np.uint64)[None, :, None]
    w = np.arange(W, dtype=np.uint64)[None, None, :]
    acc = np.zeros((len(ids), s.shape[1], W), dtype=np.uint64)
    for d in range(8):
        U = _block(idl, idh, s, side, w, d, seed)
        for half in (0, 1):
            acc = (acc | U[half]) if (q >> (2 * d + half)) & 1 else (acc & U[half])
    start = _block(idl, idh, s, side, w[:, :, :1], 8, seed)[0]
    acc[:, :, :1] = (acc[:, :, :1] & ~np.uint64(1)) | (start & np.uint64(1))
    return acc


def bits_of(words, L):
    """The first L bits of the last axis of uint64 words, bit k = bit k % 64 of word k // 64: uint8 (..., L)."""
    words = np.ascontiguousarray(words, dtype="<u8")
    flat = words.view(np.uint8).reshape(words.shape[:-1] + (8 * words.shape[-1],))
    return np.unpackbits(flat, axis=-1, bitorder="little")[..., :L]


def words_of(bits):
    """The inverse of bits_of: bits (..., L) packed into ceil(L / 64) uint64 words, the rest zero."""
    L = bits.shape[-1]
    W = (L + 63) // 64
    padded = np.zeros(bits.shape[:-1] + (64 * W,), dtype=np.uint8)
    padded[..., :L] = bits
    return np.ascontiguousarray(np.packbits(padded, axis=-1, bitorder="little")).view("<u8").astype(np.uint64)


def transmission(X, L):
    """T[k] = X[0] ^ .. ^ X[k] over the first L loci: bool (..., L)."""
    return (np.cumsum(bits_of(X, L), axis=-1, dtype=np.int64) & 1).astype(bool)


class LinkVector(IdentVector):
    def labels_of_all(self, S, L, q, seed):
        """Int32 (n_ind, 2, S, L): the labels of both sides of everyone (rows outside the live set stay -1)."""
        n, W = len(self.ind), (L + 63) // 64
        lab = np.full((n, 2, S, L), -1, dtype=np.int32)
        lab[self._allele_at, self.alleles[:, 1]] = np.arange(self.n_labels, dtype=np.int32)[:, None, None]
        sims = np.arange(S)
        for k in range(1, self.levels):
            x = np.flatnonzero(self.level == k)
            for side, parent in enumerate((self.fa, self.mo)):
                xs = x[parent[x] >= 0]
                if not len(xs):
                    continue
                p = parent[xs]
                T = transmission(crossover_words(self.ind[xs], side, sims, W, q, seed), L)
                out = np.empty((len(xs), S, L), dtype=np.int32)
                for locus in range(L):
                    out[:, :, locus] = np.where(T[:, :, locus], lab[p, 0, :, locus], lab[p, 1, :, locus])
                lab[xs, side] = out
        return lab

    def labels(self, S, L, q, seed):
        """Int32 (n_pro, 2, S, L)."""
        return np.ascontiguousarray(self.labels_of_all(S, L, q, seed)[self.pro])


def sums_of(labels):
    """Int64 (n_pro, n_pro, 6) from the probands' labels (n_pro, 2, S, L): sum m, sum m^2, sum n1, sum n2, sum g, sum [n1 > 0]."""
    n, _, S, L = labels.shape
    assert labels.min() >= 0
    out = np.zeros((n, n, 6), dtype=np.int64)
    c, d = labels[:, 0], labels[:, 1]
    edge = np.zeros((n, S, 1), dtype=np.int8)
    for i in range(n):
        a, b = labels[i, 0][None], labels[i, 1][None]
        ac, ad, bc, bd = a == c, a == d, b == c, b == d
        e = ac.astype(np.int64) + ad + bc + bd
        shared, two = e > 0, (ac & bd) | (ad & bc)
        m, n1, n2 = e.sum(axis=-1), shared.sum(axis=-1), two.sum(axis=-1)
        g = (np.diff(np.concatenate([edge, shared.astype(np.int8), edge], axis=-1), axis=-1) == 1).sum(axis=-1)
        out[i] = np.stack([m.sum(axis=1), (m * m).sum(axis=1), n1.sum(axis=1), n2.sum(axis=1), g.sum(axis=1), (n1 > 0).sum(axis=1)], axis=-1)
    return out
