"""Oracle of gen.phiNearest / genphi_result_nearest: for every given row i of a kinship matrix its k best candidates among the
columns j != i, by larger Phi[i, j] first and smaller j first among equal values.  Two selections that share nothing:
`nearest_literal` sorts Python tuples (-value, column) row by row, `nearest_numpy` is one vectorised lexsort; the tests check
them against each other before they use the fast one on large matrices.  Only comparisons and copies: every check is
np.array_equal."""
import numpy as np


def nearest_literal(phi_rows, k, row_begin=0):
    """(cols int32 (rows, k), values float32 (rows, k)).  phi_rows: rows [row_begin, row_begin + len(phi_rows)) of the N x N
    matrix (len(phi_rows[0]) = N); columns are 0-based positions in the full matrix."""
    phi_rows = np.asarray(phi_rows, dtype=np.float32)
    nr, n = phi_rows.shape
    assert 1 <= k <= n - 1
    cols, vals = np.empty((nr, k), dtype=np.int32), np.empty((nr, k), dtype=np.float32)
    for r in range(nr):
        i = row_begin + r
        best = sorted((-float(phi_rows[r, j]), j) for j in range(n) if j != i)[:k]
        for c, (_, j) in enumerate(best):
            cols[r, c] = j
            vals[r, c] = phi_rows[r, j]
    return cols, vals


def nearest_numpy(phi_rows, k, row_begin=0):
    phi_rows = np.asarray(phi_rows, dtype=np.float32)
    nr, n = phi_rows.shape
    assert 1 <= k <= n - 1
    r = np.repeat(np.arange(nr), n)
    j = np.tile(np.arange(n), nr)
    off = j != r + row_begin                                                     # the candidates: n - 1 per row
    r, j = r[off], j[off]
    order = np.lexsort((j, -phi_rows[r, j].astype(np.float64), r))              # by row, then larger value, then smaller column
    cols = j[order].reshape(nr, n - 1)[:, :k].astype(np.int32)
    return cols, phi_rows[np.arange(nr)[:, None], cols]


def same(a, b):
    """Two (cols, values) pairs hold the same bytes (values compared as bit patterns)."""
    return (all(x.dtype == y.dtype and x.shape == y.shape for x, y in zip(a, b)) and np.array_equal(a[0], b[0]) and
            np.array_equal(np.asarray(a[1]).view(np.int32), np.asarray(b[1]).view(np.int32)))
