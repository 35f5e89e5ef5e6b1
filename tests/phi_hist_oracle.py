"""Oracle of gen.phiHist / gen.phiQuantile and of genphi_result_hist / genphi_result_select (include/genphi.h), in plain numpy: the
pairs (i, j), i < j < N, of the given rows of a kinship matrix (phi_rows[k] is row row_begin + k, all N columns), each once, never
the diagonal; values compared as float64.

hist: bin b holds edges[b] <= x < edges[b + 1], the last bin also x == edges[-1]; `below` counts x < edges[0], `above` x > edges[-1].
With labels (-1 = in no group) the tables are (G, G, bins) / (G, G) and symmetric: [a, b] counts the pairs with one member in a and
the other in b; a pair with an unlabelled member counts nowhere.  Two forms: searchsorted on the widened upper triangle, and a loop
that restates the definition for tiny inputs.  select: the entries of the given 0-based ranks of the pairs sorted ascending, float32.
quantile: numpy's "linear" method written out on those order statistics."""
import math

import numpy as np


def _pairs(phi_rows, row_begin):
    phi_rows = np.asarray(phi_rows, dtype=np.float32)
    nr, n = phi_rows.shape
    k, j = np.nonzero(np.arange(n)[None, :] > (row_begin + np.arange(nr))[:, None])
    return k + row_begin, j, phi_rows[k, j]


def hist(phi_rows, edges, labels=None, n_groups=None, row_begin=0):
    """(counts, below, above): int64; below / above are ints without labels."""
    edges = np.asarray(edges, dtype=np.float64)
    bins = len(edges) - 1
    i, j, x = _pairs(phi_rows, row_begin)
    x = x.astype(np.float64)
    k = np.searchsorted(edges, x, side="right")
    k = np.where((k == bins + 1) & (x == edges[-1]), bins, k)
    if labels is None:
        t = np.bincount(k, minlength=bins + 2).astype(np.int64)
        return t[1:bins + 1].copy(), int(t[0]), int(t[bins + 1])
    labels = np.asarray(labels, dtype=np.int64)
    g = int(n_groups) if n_groups is not None else int(labels.max()) + 1
    a, b = labels[i], labels[j]
    keep = (a >= 0) & (b >= 0)
    lo, hi = np.minimum(a[keep], b[keep]), np.maximum(a[keep], b[keep])
    t = np.bincount((lo * g + hi) * (bins + 2) + k[keep], minlength=g * g * (bins + 2)).astype(np.int64).reshape(g, g, bins + 2)
    t = t + np.transpose(np.triu(np.transpose(t, (2, 0, 1)), 1), (2, 1, 0))           # mirror the strict upper part
    return t[:, :, 1:bins + 1].copy(), t[:, :, 0].copy(), t[:, :, bins + 1].copy()


def hist_loop(phi_rows, edges, labels=None, n_groups=None, row_begin=0):
    """The definition, pair by pair and edge by edge (tiny inputs only)."""
    phi_rows = np.asarray(phi_rows, dtype=np.float32)
    nr, n = phi_rows.shape
    bins = len(edges) - 1
    g = 1 if labels is None else (int(n_groups) if n_groups is not None else int(max(labels)) + 1)
    counts, below, above = np.zeros((g, g, bins), dtype=np.int64), np.zeros((g, g), dtype=np.int64), np.zeros((g, g), dtype=np.int64)
    for k in range(nr):
        i = row_begin + k
        for j in range(i + 1, n):
            a, b = (0, 0) if labels is None else (int(labels[i]), int(labels[j]))
            if a < 0 or b < 0:
                continue
            x = float(phi_rows[k, j])
            cells = {(a, b), (b, a)}
            if x < edges[0]:
                for c in cells:
                    below[c] += 1
            elif x > edges[bins]:
                for c in cells:
                    above[c] += 1
            else:
                hit = [q for q in range(bins) if edges[q] <= x and (x < edges[q + 1] or (q == bins - 1 and x == edges[bins]))]
                assert len(hit) == 1
                for c in cells:
                    counts[c][hit[0]] += 1
    if labels is None:
        return counts[0, 0], int(below[0, 0]), int(above[0, 0])
    return counts, below, above


def n_pairs(n, row_begin, row_end):
    return sum(n - 1 - i for i in range(row_begin, row_end))


def total(counts, below, above):
    """The pairs a histogram counted: bins + below + above over a <= b."""
    if np.ndim(below) == 0:
        return int(counts.sum()) + below + above
    upper = np.triu(np.ones(below.shape, dtype=bool))
    return int(counts[upper].sum() + below[upper].sum() + above[upper].sum())


def select(phi_rows, ranks, row_begin=0):
    s = np.sort(_pairs(phi_rows, row_begin)[2])
    return s[np.asarray(ranks, dtype=np.int64)]


def quantile(phi_rows, q, row_begin=0):
    s = np.sort(_pairs(phi_rows, row_begin)[2]).astype(np.float64)
    out = []
    for v in np.atleast_1d(np.asarray(q, dtype=np.float64)):
        h = v * (len(s) - 1)
        lo, hi = s[int(math.floor(h))], s[int(math.ceil(h))]
        out.append(lo + (hi - lo) * (h - math.floor(h)))
    return np.array(out, dtype=np.float64)


def same(got, ref):
    """(counts, below, above) bit for bit."""
    return all(np.array_equal(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)) and np.shape(a) == np.shape(b) for a, b in zip(got, ref))
