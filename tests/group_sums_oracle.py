"""Oracle of genphi_result_group_sums from a host matrix, and the comparison rule of its tests.

sums[a][b] = math.fsum of the Float32 entries Phi[i][j] with label[i] == a (i among the given rows) and label[j] == b;
diag[a] = math.fsum of Phi[i][i] over those rows.  math.fsum returns the exact sum correctly rounded, whatever the order.

Comparison rule (derived, not measured).  Every kinship is >= 0, so a Float64 sum of n terms taken in ANY order is within
gamma(n) = (n - 1) u / (1 - (n - 1) u) relative of the exact sum, u = 2^-53 (Higham, Accuracy and Stability of Numerical
Algorithms, 4.2: n - 1 additions, each of relative error at most u, no cancellation).  The oracle adds its own rounding of
at most u, which the rule leaves out on purpose: it is the tighter statement.  Where the terms are dyadic numbers of few
bits (pedigrees of a few generations) every partial sum is exact in Float64 and the device must EQUAL the oracle.
"""
import math

import numpy as np

U = 2.0 ** -53


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    k = np.maximum(n - 1, 0) * U
    return k / (1 - k)


def group_sums(phi, labels, n_groups, row_begin=0):
    """(sums, diag, rows_in_group, cols_in_group) of the rows phi[k] = Phi[row_begin + k] (phi: n_rows x N)."""
    phi = np.asarray(phi, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    nr, n = phi.shape
    assert len(labels) == n and row_begin + nr <= n
    row_labels = labels[row_begin:row_begin + nr]
    cols = np.bincount(labels[labels >= 0], minlength=n_groups)
    rows = np.bincount(row_labels[row_labels >= 0], minlength=n_groups)
    sums, diag = np.zeros((n_groups, n_groups)), np.zeros(n_groups)
    col_order = np.argsort(np.where(labels < 0, n_groups, labels), kind="stable")
    col_at = np.concatenate([[0], np.cumsum(cols)])
    row_order = np.argsort(np.where(row_labels < 0, n_groups, row_labels), kind="stable")
    row_at = np.concatenate([[0], np.cumsum(rows)])
    col_groups = [b for b in range(n_groups) if cols[b]]
    by_col = phi[:, col_order]
    for a in range(n_groups):
        if not rows[a]:
            continue
        mine = row_order[row_at[a]:row_at[a + 1]]
        diag[a] = math.fsum(phi[mine, row_begin + mine].tolist())
        slab = by_col[mine]
        if len(mine) == 1:
            row = slab[0].tolist()
            for b in col_groups:
                sums[a, b] = math.fsum(row[col_at[b]:col_at[b + 1]])
        else:
            for b in col_groups:
                sums[a, b] = math.fsum(slab[:, col_at[b]:col_at[b + 1]].ravel().tolist())
    return sums, diag, rows.astype(np.int64), cols.astype(np.int64)


def assert_within_rule(got_sums, got_diag, ref, exact=False):
    """The rule above, entry by entry: block [a][b] has rows[a] * cols[b] terms, diag[a] has rows[a]."""
    sums, diag, rows, cols = ref
    if exact:
        assert np.array_equal(got_sums, sums), "sums differ at %s" % (np.argwhere(got_sums != sums)[:4].tolist(),)
        assert np.array_equal(got_diag, diag), "diag differs at %s" % (np.argwhere(got_diag != diag)[:4].tolist(),)
        return
    bound = gamma(np.outer(rows, cols)) * sums
    bad = np.argwhere(~(np.abs(got_sums - sums) <= bound))
    assert len(bad) == 0, "sums%s = %r, oracle %r, bound %r" % (tuple(bad[0]), got_sums[tuple(bad[0])], sums[tuple(bad[0])], bound[tuple(bad[0])])
    bound = gamma(rows) * diag
    bad = np.argwhere(~(np.abs(got_diag - diag) <= bound))
    assert len(bad) == 0, "diag%s = %r, oracle %r" % (tuple(bad[0]), got_diag[tuple(bad[0])], diag[tuple(bad[0])])


def mean_table(ref):
    """(mean, bound): the table of phi_mean_groups from the oracle's sums, and what the rule allows a device table to differ by.
    mean[a][a] = (S - D) / (n (n - 1)): the device's S and D are within gamma(n n) S and gamma(n) D, the subtraction and the
    division round once each (2 u of the result, doubled here to cover the oracle's own three roundings)."""
    sums, diag, rows, cols = ref
    n = cols.astype(np.float64)
    den = np.outer(n, n)
    np.fill_diagonal(den, n * (n - 1))
    num = sums.copy()
    np.fill_diagonal(num, np.diagonal(sums) - diag)
    err = gamma(np.outer(rows, cols)) * sums
    err[np.diag_indices_from(err)] += gamma(rows) * diag
    mean, bound = np.full(sums.shape, np.nan), np.full(sums.shape, np.nan)
    np.divide(num, den, out=mean, where=den > 0)
    np.divide(err, den, out=bound, where=den > 0)
    return mean, bound + 4 * U * np.abs(mean)
