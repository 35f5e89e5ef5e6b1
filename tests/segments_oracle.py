"""The CPU reference of gen.simuSegments (the definition is the text in include/genphi.h, genphi_seg_*), in numpy on single loci: no
words, no count-trailing-zeros, no carried state.  From the labels of tests/link_oracle.py it forms `shared` per pair as sums_of
does, finds the runs by np.diff on the padded row, then bins, censors and reduces them.

runs_of_rows     start and length of every run of every row of a bool array (..., L)
reduce_bits      one chromosome given as bits: the (n_bins + 2, 3) table and the three per-pair numbers (what genphi_seg_host adds)
runs_of          every run of every ordered pair of probands: i, j, simulation, start, length
segments_of      (hist, pairs) of a request: hist (G, G, n_bins + 2, 3) over the pairs i < j, pairs (n, n, 3)
run_classes      how many runs of the pairs i < j cross a word border, are censored, span the chromosome, ..: what a test asserts
                 about its own fixture
"""
import numpy as np


def runs_of_rows(shared):
    """(row index, start, length) of every maximal run of True along the last axis; rows are the flattened leading axes."""
    shared = np.asarray(shared, dtype=bool)
    L = shared.shape[-1]
    flat = shared.reshape(-1, L).astype(np.int8)
    edge = np.zeros((flat.shape[0], 1), dtype=np.int8)
    d = np.diff(np.concatenate([edge, flat, edge], axis=1), axis=1)          # (rows, L + 1): +1 where a run starts, -1 one past its end
    row, start = np.nonzero(d == 1)
    row_e, stop = np.nonzero(d == -1)                                        # both in (row, position) order: the k-th start meets the k-th end
    assert np.array_equal(row, row_e)
    return row.astype(np.int64), start.astype(np.int64), (stop - start).astype(np.int64)


def bin_of(edges, length):
    """The column of a length: 0 below edges[0], 1 + b in bin b, len(edges) at or above the last edge."""
    return np.searchsorted(np.asarray(edges, dtype=np.int64), length, side="right")


def reduce_bits(bits, edges, min_loci=1):
    """One pair in one simulation, `any` given as L bits: int64 (n_bins + 2, 3) and int64 (3,)."""
    bits = np.asarray(bits, dtype=bool)
    L = len(bits)
    _, start, length = runs_of_rows(bits[None])
    hist = np.zeros((len(edges) + 1, 3), dtype=np.int64)
    k = bin_of(edges, length)
    censored = (start == 0) | (start + length == L)
    np.add.at(hist[:, 0], k, 1)
    np.add.at(hist[:, 1], k, length)
    np.add.at(hist[:, 2], k, censored.astype(np.int64))
    over = length >= min_loci
    return hist, np.array([over.sum(), length[over].sum(), length.max(initial=0)], dtype=np.int64)


def _shared_rows(labels, i):
    """bool (n, S, L): the loci at which proband i shares an allele with every proband j."""
    a, b = labels[i, 0][None], labels[i, 1][None]
    c, d = labels[:, 0], labels[:, 1]
    return (a == c) | (a == d) | (b == c) | (b == d)


def runs_of(labels):
    """int64 arrays (i, j, s, start, length): every run of every ordered pair (the diagonal included)."""
    n, _, S, L = labels.shape
    assert labels.min() >= 0
    out = []
    for i in range(n):
        row, start, length = runs_of_rows(_shared_rows(labels, i))
        out.append((np.full(len(row), i, dtype=np.int64), row // S, row % S, start, length))
    return tuple(np.concatenate(c) for c in zip(*out))


def segments_of(labels, edges, min_loci=1, groups=None):
    """(hist, pairs) from the probands' labels (n, 2, S, L).  groups: None or a label per list position, -1 = counts nowhere; the
    number of groups is max(groups) + 1, at least 1."""
    n, _, S, L = labels.shape
    edges = np.asarray(edges, dtype=np.int64)
    g = np.zeros(n, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    G = max(int(g.max(initial=-1)) + 1, 1)
    i, j, s, start, length = runs_of(labels)
    pairs = np.zeros((n, n, 3), dtype=np.int64)
    over = length >= min_loci
    np.add.at(pairs[:, :, 0], (i[over], j[over]), 1)
    np.add.at(pairs[:, :, 1], (i[over], j[over]), length[over])
    longest = np.zeros((n, n, S), dtype=np.int64)
    np.maximum.at(longest, (i, j, s), length)
    pairs[:, :, 2] = longest.sum(axis=2)
    hist = np.zeros((G, G, len(edges) + 1, 3), dtype=np.int64)
    keep = (i < j) & (g[i] >= 0) & (g[j] >= 0)
    a, b = np.minimum(g[i], g[j])[keep], np.maximum(g[i], g[j])[keep]
    k = bin_of(edges, length[keep])
    censored = ((start == 0) | (start + length == L))[keep].astype(np.int64)
    np.add.at(hist[..., 0], (a, b, k), 1)
    np.add.at(hist[..., 1], (a, b, k), length[keep])
    np.add.at(hist[..., 2], (a, b, k), censored)
    for x in range(G):
        for y in range(x):
            hist[x, y] = hist[y, x]
    return hist, pairs


def run_classes(labels):
    """dict of counts over the runs of the pairs i < j."""
    L = labels.shape[3]
    i, j, _, start, length = runs_of(labels)
    up = i < j
    start, length = start[up], length[up]
    last = start + length - 1
    first_c, last_c = start == 0, last == L - 1
    return {
        "segments": int(up.sum()),
        "lengths": int(len(np.unique(length))),
        "cross": int((start // 64 != last // 64).sum()),
        "censored": int((first_c | last_c).sum()),
        "spanning": int((first_c & last_c).sum()),
        "interior": int((~first_c & ~last_c).sum()),
        "end_at_63": int(((last % 64 == 63) & ~last_c).sum()),
        "start_at_0": int(((start % 64 == 0) & (start > 0)).sum()),
    }
