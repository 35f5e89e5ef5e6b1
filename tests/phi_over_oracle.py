"""Oracle of gen.phiOver / genphi_result_over: the pairs (i, j), i < j, of the given rows of a kinship matrix with
float64(Phi[i, j]) >= threshold, sorted by row, then column.  `over` is the definition as a plain double loop, `over_numpy` the
same selection vectorised; the tests check them against each other before they use the fast one on large matrices.  Only
comparisons and copies: every check is np.array_equal."""
import numpy as np


def over(phi_rows, threshold, row_begin=0):
    """(rows int32, cols int32, values float32).  phi_rows: rows [row_begin, row_begin + len(phi_rows)) of the N x N matrix
    (len(phi_rows[0]) = N); positions are 0-based in the full matrix."""
    phi_rows = np.asarray(phi_rows, dtype=np.float32)
    t = float(threshold)
    rows, cols, vals = [], [], []
    for k in range(phi_rows.shape[0]):
        i = row_begin + k
        for j in range(i + 1, phi_rows.shape[1]):
            if float(phi_rows[k, j]) >= t:
                rows.append(i)
                cols.append(j)
                vals.append(phi_rows[k, j])
    return np.array(rows, dtype=np.int32), np.array(cols, dtype=np.int32), np.array(vals, dtype=np.float32)


def over_numpy(phi_rows, threshold, row_begin=0):
    phi_rows = np.asarray(phi_rows, dtype=np.float32)
    nr, n = phi_rows.shape
    right = np.arange(n)[None, :] > (row_begin + np.arange(nr))[:, None]            # strictly right of the diagonal
    k, j = np.nonzero(right & (phi_rows.astype(np.float64) >= float(threshold)))     # (row-major: by row, then column)
    return (k + row_begin).astype(np.int32), j.astype(np.int32), phi_rows[k, j]


def same(a, b):
    """Two (rows, cols, values) triples hold the same bytes (values compared as bit patterns)."""
    return (all(x.dtype == y.dtype and x.shape == y.shape for x, y in zip(a, b)) and np.array_equal(a[0], b[0]) and
            np.array_equal(a[1], b[1]) and np.array_equal(np.asarray(a[2]).view(np.int32), np.asarray(b[2]).view(np.int32)))
