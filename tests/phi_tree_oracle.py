"""The oracle of gen.phiTree (include/genphi.h: genphi_result_tree) in plain numpy and a Python loop: Kruskal's rule, literally.  Every
pair i < j of the upper triangle with float64(kinship) >= floor is listed and sorted with np.lexsort on (j, i, -kinship); an edge is
taken iff its ends carry different labels, and taking it relabels the smaller side.  It shares no code and no trick with the package:
no rounds, no keys, no union-find.  Before the Python loop sees a chunk of the sorted list, the edges whose ends already share a label
are dropped in numpy, which keeps 2,500 probands at a few seconds."""
import numpy as np

CHUNK = 20_000


def floor_of(floor):
    """None is the smallest positive Float32."""
    return float(np.finfo(np.float32).smallest_subnormal) if floor is None else float(floor)


def forest(phi, floor=None):
    """(row int32, col int32, kinship float32, n_trees) of the square Float32 host matrix phi (no padding columns)."""
    phi = np.asarray(phi)
    assert phi.dtype == np.float32 and phi.ndim == 2 and phi.shape[0] == phi.shape[1]
    n = len(phi)
    t = floor_of(floor)
    assert t == t
    i, j = np.nonzero(np.triu(np.ones((n, n), dtype=bool), 1))
    w = phi[i, j].astype(np.float64)
    ok = w >= t
    i, j, w = i[ok], j[ok], w[ok]
    order = np.lexsort((j, i, -w))
    i, j = i[order], j[order]
    label = np.arange(n)
    members = {v: [v] for v in range(n)}
    rows, cols = [], []
    for start in range(0, len(i), CHUNK):
        ci, cj = i[start:start + CHUNK], j[start:start + CHUNK]
        for e in np.flatnonzero(label[ci] != label[cj]).tolist():
            a, b = int(label[ci[e]]), int(label[cj[e]])
            if a == b:
                continue
            if len(members[a]) < len(members[b]):
                a, b = b, a
            label[members[b]] = a
            members[a] += members.pop(b)
            rows.append(int(ci[e]))
            cols.append(int(cj[e]))
    rows, cols = np.asarray(rows, dtype=np.int32), np.asarray(cols, dtype=np.int32)
    return rows, cols, phi[rows, cols], len(members)


def same(got, want):
    """got = (row, col, kinship, ...) equals the oracle's, kinships as bit patterns."""
    return (got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float32 and
            np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and
            np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)))


def labels_of(n, row, col):
    """int32 (n,): the smallest position of every vertex's component in the graph of the given edges, by repeated relabelling."""
    label = np.arange(n, dtype=np.int32)
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    while True:
        low = np.minimum(label[row], label[col])
        new = label.copy()
        np.minimum.at(new, row, low)
        np.minimum.at(new, col, low)
        if np.array_equal(new, label):
            return label
        label = new


def log2_ceil(n):
    return 0 if n <= 1 else int(n - 1).bit_length()
