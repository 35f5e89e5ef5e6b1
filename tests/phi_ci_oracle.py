"""CPU reference for the bootstrap of mean kinship (gen.phiCI / gen.fCI; the definition is the text in include/genphi.h).  It shares
no code with the library: the draws come from simu_oracle.philox_vector, the high half of the 128-bit product from Python
integers, and the statistic is computed literally on the resampled matrix Phi[s, s]."""
import math

import numpy as np

from simu_oracle import philox_vector

# (N, seed, resample, draw) -> position: the known answers of include/genphi.h
KNOWN_DRAWS = [
    ((140, 0, 0, 0), 95),
    ((140, 0, 0, 1), 115),
    ((100000, 0x123456789ABCDEF, 4999, 99999), 67714),
]


def draws(n, seed, r):
    """The n drawn positions of resample r, in draw order: int64 (n,)."""
    pairs = (n + 1) // 2
    o0, o1, o2, o3 = philox_vector(np.arange(pairs, dtype=np.uint64), r, 0, 2, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    words = np.empty(2 * pairs, dtype=np.uint64)
    words[0::2] = o0 | (o1 << np.uint64(32))
    words[1::2] = o2 | (o3 << np.uint64(32))
    return np.array([(int(w) * n) >> 64 for w in words[:n]], dtype=np.int64)


def counts(n, seed, first, n_boot):
    """int32 (n_boot, n): how often each position was drawn in the resamples first .. first + n_boot - 1."""
    return np.stack([np.bincount(draws(n, seed, first + b), minlength=n) for b in range(n_boot)]).astype(np.int32)


def _total(values, exact):
    """The sum of a Float64 array: math.fsum (the correctly rounded exact sum), or numpy's sum where the caller has asserted
    exact_precondition -- then every partial sum in Float64 is exact and any order gives fsum's value, much faster."""
    return float(values.sum()) if exact else math.fsum(values.tolist())


def quad_self_literal(phi, s, row_begin=0, row_end=None, exact=False):
    """(quad, self) of one resample given its draws s, restricted to the drawn rows in [row_begin, row_end): the entries of
    Phi[s, s] in Float64, added up."""
    phi = np.asarray(phi, dtype=np.float64)
    row_end = len(phi) if row_end is None else row_end
    rows = s[(s >= row_begin) & (s < row_end)]
    return _total(phi[np.ix_(rows, s)].ravel(), exact), _total(phi[rows, rows], exact)


def theta_literal(phi, s, exact=False):
    """phiMean of the resampled matrix Phi[s, s]: its off-diagonal POSITIONS added up (the diagonal positions set to zero, which
    adds nothing), over N (N - 1)."""
    phi = np.asarray(phi, dtype=np.float64)
    n = len(s)
    m = phi[np.ix_(s, s)]
    np.fill_diagonal(m, 0.0)
    return _total(m.ravel(), exact) / (n * (n - 1))


def bootstrap(phi, seed, first, n_boot, row_begin=0, row_end=None, exact=False):
    """(quad, self, theta) float64 arrays of the resamples first .. first + n_boot - 1; theta is NaN for a row shard."""
    phi = np.asarray(phi, dtype=np.float64)
    n = len(phi)
    whole = row_begin == 0 and row_end in (None, n)
    out = np.full((3, n_boot), math.nan, dtype=np.float64)
    for b in range(n_boot):
        s = draws(n, seed, first + b)
        if whole:                                              # one gather serves both: Phi[s, s], then its diagonal zeroed
            m = phi[np.ix_(s, s)]
            out[0, b], out[1, b] = _total(m.ravel(), exact), _total(phi[s, s], exact)
            np.fill_diagonal(m, 0.0)
            out[2, b] = _total(m.ravel(), exact) / (n * (n - 1))
        else:
            out[0, b], out[1, b] = quad_self_literal(phi, s, row_begin, row_end, exact)
    return out[0], out[1], out[2]


def exact_precondition(phi, cnt):
    """True when every partial sum of quad is exact in Float64 whatever the order: every entry of Phi a multiple of 2^-k and
    N^2 max(c)^2 2^k < 2^53 (all terms are >= 0 and multiples of 2^-k, so every partial sum is a multiple of 2^-k below 2^(53 - k))."""
    phi = np.asarray(phi, dtype=np.float64)
    if not np.all(phi >= 0) or phi.max() > 1:
        return False
    k = 0
    while k <= 60 and not np.array_equal(np.floor(phi * 2.0 ** k), phi * 2.0 ** k):
        k += 1
    if k > 60:
        return False
    n, cmax = len(phi), int(np.max(cnt))
    return n * n * cmax * cmax * 2 ** k < 2 ** 53
