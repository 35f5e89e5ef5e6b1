"""Exact kinship coefficients as Python integers: the reference the Float64 sweep and the oracle's Float64 mode are held to.

Every kinship coefficient of a pedigree is a dyadic rational.  With all of them scaled by 2^S, S = 2 * (generations) + 3,
they are integers, and the textbook recursion over the individuals in an order where parents come first

    K[i][i] = (1 + K[f][m]) / 2,        K[i][j] = (K[f][j] + K[m][j]) / 2   (j before i; an unknown parent's row is 0)

only adds and halves them.  Every halving is asserted exact, so a result is the kinship itself, not an approximation.  This
module shares nothing with the planner or the oracle's levelisation: one pass over the whole pedigree in its own
parents-first order.  Dense (N x N Python integers): meant for N up to a few thousand.

`value(i, j) / 2^S` as int / int true division is the correctly rounded double (subnormals included); np.float32 of it is
within half an ulp of the correctly rounded Float32, enough for the 1-ulp Float32 checks.
"""
from fractions import Fraction

import numpy as np


class ExactKinship:
    def __init__(self, ind, father, mother):
        ind = [int(x) for x in ind]
        father = [int(x) for x in father]
        mother = [int(x) for x in mother]
        n = len(ind)
        pos = {x: k for k, x in enumerate(ind)}
        assert len(pos) == n, "duplicate ID"
        fa = [pos[x] if x else -1 for x in father]
        mo = [pos[x] if x else -1 for x in mother]
        # generation depth (founders 1) by an explicit stack, and a parents-first order (depth, then file position)
        depth = [0] * n
        for s in range(n):
            stack = [s]
            while stack:
                x = stack[-1]
                if depth[x]:
                    stack.pop()
                    continue
                todo = [q for q in (fa[x], mo[x]) if q >= 0 and not depth[q]]
                if todo:
                    stack.extend(todo)
                    continue
                depth[x] = 1 + max([depth[q] for q in (fa[x], mo[x]) if q >= 0], default=0)
                stack.pop()
        order = sorted(range(n), key=lambda k: (depth[k], k))
        self.generations = max(depth, default=0)
        self.S = S = 2 * self.generations + 3
        one = 1 << S
        # K[a][b] over positions in `order`; row / column n is the unknown parent (all zero)
        at = {k: a for a, k in enumerate(order)}
        K = np.zeros((n + 1, n + 1), dtype=object)
        K[:, :] = 0
        for a, k in enumerate(order):
            f = at[fa[k]] if fa[k] >= 0 else n
            m = at[mo[k]] if mo[k] >= 0 else n
            row = K[f, :a] + K[m, :a]
            assert not np.any(row & 1), "inexact halving"
            row = row >> 1
            K[a, :a] = row
            K[:a, a] = row
            d = one + K[f, m]
            assert d & 1 == 0, "inexact halving"
            K[a, a] = d >> 1
        self._K, self._at, self._pos, self.n = K, at, pos, n

    def _idx(self, ids):
        return np.array([self._at[self._pos[int(x)]] for x in np.atleast_1d(ids)], dtype=np.int64)

    def scaled(self, ids_a, ids_b):
        """Kinships of ids_a x ids_b, as Python integers scaled by 2^S (object array)."""
        return self._K[np.ix_(self._idx(ids_a), self._idx(ids_b))]

    def float64(self, ids_a, ids_b=None):
        """Kinships of ids_a x ids_b (ids_b = ids_a by default), correctly rounded to float64."""
        ids_b = ids_a if ids_b is None else ids_b
        den = 1 << self.S
        sub = self.scaled(ids_a, ids_b)
        return np.array([[int(v) / den for v in r] for r in sub], dtype=np.float64).reshape(sub.shape)

    def pairs64(self, ids_a, ids_b):
        """Kinship of each pair (ids_a[k], ids_b[k]), correctly rounded to float64."""
        den = 1 << self.S
        ia, ib = self._idx(ids_a), self._idx(ids_b)
        return np.array([int(self._K[a, b]) / den for a, b in zip(ia, ib)], dtype=np.float64)


def level_steps(ped_oracle, pro):
    """Number of level steps of the sweep for `pro` (cuts - 1), the L of the Float64 error bound 2 L 2^-53."""
    return len(ped_oracle.levels(pro)[0]) - 1


def rel_err_bound(n_steps):
    """The bound the Float64 sweep is held to: every entry is a sum of non-negative terms, every level adds at most two
    roundings of relative size 2^-53 along any path into it, and the scalings by 1/2 and 1/4 are exact (normal range)."""
    return 2.0 * n_steps * 2.0 ** -53


def max_rel_err(got, scaled, S):
    """max |got - exact| / exact over the entries whose exact kinship (`scaled` / 2^S, integers) is not 0, evaluated in exact
    rational arithmetic; asserts got == 0 exactly where the kinship is 0."""
    got = np.asarray(got, dtype=np.float64)
    worst = Fraction(0)
    for g, k in zip(got.ravel().tolist(), np.asarray(scaled, dtype=object).ravel().tolist()):
        k = int(k)
        if k == 0:
            assert g == 0.0, "non-zero where the kinship is exactly 0"
            continue
        e = abs(Fraction(g) * (1 << S) - k) / k
        if e > worst:
            worst = e
    return float(worst)
