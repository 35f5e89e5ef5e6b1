"""gen.phiTree without a GPU: genphi_tree_host (the rounds of the device with the key arithmetic of its kernels, csrc/tree.cpp and
csrc/tree_keys.h) and gen.phiTree on a square host matrix (Kruskal in numpy) against tests/phi_tree_oracle.py, and the invariants of
include/genphi.h against tests/phi_clusters_oracle.py.  Every comparison is np.array_equal; kinships are compared as bit patterns."""
import ctypes
import math
import os

import numpy as np
import pytest

import phi_clusters_oracle as CO
import phi_tree_oracle as TO

I32P, F32P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
FLOORS = (None, 0.0, -math.inf, math.inf)


def _tie_matrix(n, seed=20261021):
    """A symmetric Float32 matrix with few distinct values, so many ties, and zeros."""
    r = np.random.default_rng([seed, n])
    m = r.choice(np.array([0, 0, 0, 2.0 ** -8, 2.0 ** -6, 2.0 ** -4, 2.0 ** -3, 0.25], dtype=np.float32), size=(n, n))
    m = np.triu(m, 1)
    m = (m + m.T).astype(np.float32)
    np.fill_diagonal(m, 0.5)
    return m


def _cycle(order):
    """Equal weights 0.125 between neighbours on a ring through the positions as listed in `order`, zeros elsewhere."""
    n = len(order)
    m = np.zeros((n, n), dtype=np.float32)
    at = np.empty(n, dtype=np.int64)
    at[np.asarray(order)] = np.arange(n)                                       # at[v] = the position of ring vertex v
    for v in range(n):
        a, b = at[v], at[(v + 1) % n]
        m[a, b] = m[b, a] = 0.125
    np.fill_diagonal(m, 0.5)
    return m


def _floors_between(m):
    """The floors of every test plus a few drawn from the matrix: distinct off-diagonal values and a point between two of them."""
    n = len(m)
    out = list(FLOORS)
    if n >= 2:
        d = np.unique(m[np.triu_indices(n, 1)])
        out += [float(d[len(d) // 2]), float(d[-1]), float(np.nextafter(d[-1], np.float32(2)))]
        if len(d) >= 2:
            out.append((float(d[0]) + float(d[1])) / 2)
    return out


def _check(gen, m, floor):
    """Both host forms give the oracle's forest of m at `floor`; the invariants hold.  Returns the PhiTree."""
    n = len(m)
    want = TO.forest(m, floor)
    host = gen._capi.tree_host(m, floor)
    assert TO.same(host, want) and host[3] == want[3], (n, floor)
    tree = gen.phiTree(m, floor)
    assert TO.same((tree.row, tree.col, tree.kinship), want) and tree.n_trees == want[3] and tree.rounds == 0 and len(tree) == len(want[0])
    assert tree.floor == TO.floor_of(floor) and tree.pro is None and tree.pro1 is None and tree.pro2 is None
    row, col, kin, n_trees, rounds = host
    assert len(row) == n - n_trees and np.all(row < col)
    assert np.all(kin[:-1] >= kin[1:])                                           # the order: larger kinship first ...
    tie = kin[:-1] == kin[1:]
    pair = row.astype(np.int64) << 32 | col
    assert np.all(pair[:-1][tie] < pair[1:][tie])                                # ... then smaller row, then smaller column
    # invariant 5
    assert rounds <= TO.log2_ceil(n) + 1 and (rounds >= 1) == (n >= 2)
    # invariants 1 and 2 at the floor and at every distinct kinship of the list (and one step above the top)
    f = TO.floor_of(floor)
    levels = [f] + [float(x) for x in np.unique(kin) if float(x) >= f]
    if len(kin):
        levels.append(float(np.nextafter(kin[0], np.float32(2))))
    for t in levels:
        k = int(np.count_nonzero(kin.astype(np.float64) >= t))
        label = CO.components(CO.adjacency(m, t))
        assert np.array_equal(TO.labels_of(n, row[:k], col[:k]), label), (n, floor, t)
        assert k == n - len(np.unique(label))
        assert np.array_equal(tree.cut(t), label) and tree.cut(t).dtype == np.int32
    assert n_trees == len(np.unique(CO.components(CO.adjacency(m, f)))) if n else n_trees == 0
    return tree


# ---- against the oracle ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65, 257])
def test_random_matrices_with_many_ties(gen, n):
    m = _tie_matrix(n)
    for floor in _floors_between(m):
        _check(gen, m, floor)


def test_the_140_probands_of_the_committed_golden(gen):
    phi = np.load(os.path.join(os.path.dirname(__file__), "golden", "genea140_phi_oracle.npy")).astype(np.float32)
    assert phi.shape == (140, 140) and np.array_equal(phi, phi.T)
    for floor in (None, 0.0, 1 / 64, 1 / 8, math.inf):
        tree = _check(gen, phi, floor)
    assert tree.n_trees == 140 and len(tree) == 0
    assert _check(gen, phi, 0.0).n_trees == 1


def test_a_tiny_hand_matrix(gen):
    """Three probands in the shape of geneaJi's: one close pair, one proband further away."""
    m = np.array([[0.5, 0.25, 0.0625], [0.25, 0.5, 0.125], [0.0625, 0.125, 0.5]], dtype=np.float32)
    tree = _check(gen, m, None)
    assert tree.row.tolist() == [0, 1] and tree.col.tolist() == [1, 2] and tree.kinship.tolist() == [0.25, 0.125] and tree.n_trees == 1
    tree = _check(gen, m, 0.25)
    assert tree.row.tolist() == [0] and tree.col.tolist() == [1] and tree.n_trees == 2
    assert len(_check(gen, m, float(np.nextafter(np.float32(0.25), np.float32(1))))) == 0


def test_the_all_equal_matrix_gives_the_star_at_position_0(gen):
    for n in (2, 7, 130):
        m = np.full((n, n), 0.125, dtype=np.float32)
        for floor in (None, 0.0, 0.125):
            tree = _check(gen, m, floor)
            assert tree.row.tolist() == [0] * (n - 1) and tree.col.tolist() == list(range(1, n)) and tree.n_trees == 1
        assert len(_check(gen, m, 0.126)) == 0


@pytest.mark.parametrize("shuffled", [False, True])
def test_a_cycle_of_equal_weights(gen, shuffled):
    """300 equal edges in a ring: 299 of them, no cycle.  An inconsistent tie-break between the components closes the ring."""
    order = np.random.default_rng(300).permutation(300) if shuffled else np.arange(300)
    m = _cycle(order)
    tree = _check(gen, m, 0.125)
    assert len(tree) == 299 and tree.n_trees == 1 and np.all(tree.kinship == np.float32(0.125))
    assert len(set(zip(tree.row.tolist(), tree.col.tolist()))) == 299
    assert np.array_equal(TO.labels_of(300, tree.row, tree.col), np.zeros(300, dtype=np.int32))
    tree = _check(gen, m, None)
    assert len(tree) == 299
    tree = _check(gen, m, 0.0)                                                   # the zeros are edges too, after the ring's
    assert len(tree) == 299 and np.all(tree.kinship == np.float32(0.125))


def test_a_larger_floor_gives_the_prefix_that_passes_it(gen):
    m = _tie_matrix(65)
    full = gen._capi.tree_host(m, 0.0)
    for floor in (None, 2.0 ** -8, 2.0 ** -6, 0.01, 2.0 ** -3, 0.25, 0.3, math.inf):
        k = int(np.count_nonzero(full[2].astype(np.float64) >= TO.floor_of(floor)))
        part = gen._capi.tree_host(m, floor)
        assert TO.same(part, tuple(a[:k] for a in full[:3])) and part[3] == 65 - k
        tree = gen.phiTree(m, floor)
        assert TO.same((tree.row, tree.col, tree.kinship), tuple(a[:k] for a in full[:3]))


def test_a_row_pitch_with_junk_in_the_padding(gen):
    n, ld = 65, 128
    m = _tie_matrix(n)
    wide = np.full((n, ld), 7.5, dtype=np.float32)                               # junk above every entry: it would win every pick
    wide[:, ld - 1] = np.nan
    wide[:, :n] = m
    for floor in (None, 0.0, 2.0 ** -6, -math.inf):
        got = gen._capi.tree_host(wide, floor)
        assert TO.same(got, TO.forest(m, floor)) and got[4] == gen._capi.tree_host(m, floor)[4]


def test_a_threshold_between_two_float32_values(gen):
    """The comparison is float64(entry) >= floor, as gen.phiOver's."""
    lo = np.float32(0.1)
    hi = np.nextafter(lo, np.float32(1))
    m = np.zeros((5, 5), dtype=np.float32)
    m[0, 1] = m[1, 0] = m[1, 2] = m[2, 1] = lo
    m[3, 4] = m[4, 3] = hi
    np.fill_diagonal(m, 0.5)
    between = float(np.nextafter(np.float64(lo), np.inf))
    assert len(_check(gen, m, float(lo))) == 3 and len(_check(gen, m, 0.1)) == 3
    tree = _check(gen, m, between)
    assert tree.row.tolist() == [3] and tree.col.tolist() == [4]
    assert _check(gen, m, float(lo)).kinship.view(np.uint32).tolist() == [hi.view(np.uint32), lo.view(np.uint32), lo.view(np.uint32)]


# ---- what a PhiTree offers ------------------------------------------------------------------------------------------------------

def test_cut_clusters_heights_and_linkage(gen):
    m = _tie_matrix(64)
    ids = 1000 + np.arange(64)[::-1]
    tree = gen.phiTree(m, 0.0, probandIDs=ids)
    n = 64
    assert tree.n_trees == 1 and len(tree) == n - 1 and np.array_equal(tree.pro, ids)
    assert np.array_equal(tree.pro1, ids[tree.row]) and np.array_equal(tree.pro2, ids[tree.col])
    assert "64 probands" in repr(tree) and "63 edges" in repr(tree) and "1 tree " in repr(tree)
    # heights: descending, distinct, and the clusters left at each are gen.phiClusters' at that threshold
    h, left = tree.heights()
    assert h.dtype == np.float32 and left.dtype == np.int64 and np.all(h[:-1] > h[1:]) and np.array_equal(h, np.unique(tree.kinship)[::-1])
    assert left[-1] == 1 and np.all(left[:-1] > left[1:])
    for t, k in zip(h.tolist(), left.tolist()):
        ref = gen.phiClusters(m, t, probandIDs=ids)
        c = tree.clusters(t)
        assert len(c) == k == len(ref) and c.n_pairs is None and c.threshold == t and "pairs not counted" in repr(c)
        assert np.array_equal(c.label, ref.label) and np.array_equal(c.cluster, ref.cluster) and np.array_equal(c.sizes, ref.sizes)
        assert np.array_equal(c.pro, ref.pro) and [c.members(q).tolist() for q in range(len(c))] == [ref.members(q).tolist() for q in range(len(c))]
        assert np.array_equal(tree.cut(t), ref.label)
    # linkage: SciPy's convention
    z = tree.linkage()
    assert z.shape == (n - 1, 4) and z.dtype == np.float64
    assert np.array_equal(z[:, 2], 1.0 - tree.kinship.astype(np.float64)) and np.all(np.diff(z[:, 2]) >= 0)
    assert np.all(z[:, 0] < z[:, 1]) and z[-1, 3] == n
    size = {v: 1 for v in range(n)}
    leaves = {v: {v} for v in range(n)}
    for k in range(n - 1):
        a, b = int(z[k, 0]), int(z[k, 1])
        assert a in size and b in size                                           # an id is used once, and only after it was made
        size[n + k] = size.pop(a) + size.pop(b)
        leaves[n + k] = leaves.pop(a) | leaves.pop(b)
        assert z[k, 3] == size[n + k]
        ra, ca = int(tree.row[k]), int(tree.col[k])
        assert ra in leaves[n + k] and ca in leaves[n + k]                       # row k is the merge that edge k makes
    assert list(size) == [2 * n - 2] and leaves[2 * n - 2] == set(range(n))
    # a forest has no merge table; a cut below the floor is refused
    m = m.copy()
    m[63, :63] = m[:63, 63] = 0                                                  # the last proband is related to nobody
    forest = gen.phiTree(m, 0.25)
    assert forest.n_trees > 1 and "trees" in repr(forest)
    with pytest.raises(ValueError, match="trees"):
        forest.linkage()
    with pytest.raises(ValueError, match="says nothing"):
        forest.cut(0.2)
    with pytest.raises(ValueError, match="says nothing"):
        forest.clusters(0.0)
    with pytest.raises(ValueError, match="NaN"):
        forest.cut(math.nan)
    assert np.array_equal(forest.cut(math.inf), np.arange(n)) and np.array_equal(forest.cut(0.25), gen.phiClusters(m, 0.25).label)
    hf, lf = forest.heights()
    assert hf.tolist() == [0.25] and lf.tolist() == [forest.n_trees]


def test_small_matrices(gen):
    for n in (0, 1, 2):
        m = np.full((n, n), 0.25, dtype=np.float32)
        tree = gen.phiTree(m)
        assert len(tree) == max(n - 1, 0) and tree.n_trees == min(n, 1) and repr(tree)
        assert tree.cut(0.25).tolist() == [0] * n and tree.heights()[0].tolist() == [0.25] * (n - 1)
        got = gen._capi.tree_host(m)
        assert len(got[0]) == max(n - 1, 0) and got[3] == min(n, 1) and got[4] == (1 if n == 2 else 0)
        if n == 2:
            assert tree.linkage().tolist() == [[0.0, 1.0, 0.75, 2.0]]


# ---- argument errors ------------------------------------------------------------------------------------------------------------

def test_value_errors(gen):
    m = _tie_matrix(9)
    with pytest.raises(ValueError, match="NaN"):
        gen.phiTree(m, math.nan)
    with pytest.raises(ValueError, match="square"):
        gen.phiTree(m[:, :8])
    with pytest.raises(ValueError, match="square"):
        gen.phiTree(m[0])
    with pytest.raises(ValueError, match="probandIDs"):
        gen.phiTree(m, probandIDs=np.arange(8))
    with pytest.raises(ValueError, match="NaN"):
        gen._capi.tree_host(m, math.nan)
    with pytest.raises(ValueError, match="pitch"):
        gen._capi.tree_host(m[:, :8])


def test_the_c_entry_point_checks_its_arguments_and_takes_null_outputs(gen):
    L, C = gen._capi.lib(), gen._capi
    m = np.ascontiguousarray(_tie_matrix(9))
    mp = m.ctypes.data_as(F32P)

    def call(mp, n, ld, floor):
        row, col, kin = np.full(8, -7, np.int32), np.full(8, -7, np.int32), np.full(8, -7, np.float32)
        k, trees, rounds = ctypes.c_int64(-7), ctypes.c_int64(-7), ctypes.c_int32(-7)
        rc = L.genphi_tree_host(mp, n, ld, floor, row.ctypes.data_as(I32P), col.ctypes.data_as(I32P), kin.ctypes.data_as(F32P), ctypes.byref(k),
                                ctypes.byref(trees), ctypes.byref(rounds))
        return rc, row, col, kin, k.value, trees.value, rounds.value

    for args in ((mp, 9, 9, math.nan), (mp, -1, 9, 0.0), (mp, 1 << 31, 1 << 31, 0.0), (None, 9, 9, 0.0), (mp, 9, 8, 0.0)):
        rc, row, col, kin, k, trees, rounds = call(*args)
        assert rc == C.GENPHI_ERR_ARG and gen._capi.last_error()
        assert np.all(row == -7) and np.all(col == -7) and np.all(kin == -7) and (k, trees, rounds) == (-7, -7, -7)
    rc, row, col, kin, k, trees, rounds = call(None, 1, 0, 0.0)                  # n < 2: the trivial answer, the matrix is not looked at
    assert rc == 0 and (k, trees, rounds) == (0, 1, 0) and np.all(row == -7)
    rc, row, col, kin, k, trees, rounds = call(mp, 9, 9, 0.0)
    want = TO.forest(m, 0.0)
    assert rc == 0 and k == 8 and trees == 1 and TO.same((row, col, kin), want)
    assert L.genphi_tree_host(mp, 9, 9, 0.0, None, None, None, None, None, None) == 0
    k = ctypes.c_int64(-7)
    assert L.genphi_tree_host(mp, 9, 9, 0.25, None, None, None, ctypes.byref(k), None, None) == 0 and k.value == len(TO.forest(m, 0.25)[0])


def test_the_plan_has_the_method_and_the_library_the_symbols(gen):
    assert callable(gen.PhiPlan.tree) and callable(gen.phiTree)
    L = gen._capi.lib()
    assert hasattr(L, "genphi_result_tree") and hasattr(L, "genphi_tree_host")
    assert "genphi_result_tree" in gen._capi.EXPORTED_SYMBOLS and "genphi_tree_host" in gen._capi.EXPORTED_SYMBOLS
    ped = gen.genealogy(gen.geneaJi)
    pl = gen.plan(ped)
    try:
        with pytest.raises(ValueError, match="NaN"):
            pl.tree(math.nan)
        with pytest.raises(gen.GenphiDeviceError):                               # never computed: no resident result
            pl.tree(0.1)
    finally:
        pl.close()
    pl = gen.plan(ped, [29])                                                     # one proband: the trivial answer, no device needed
    try:
        row, col, kin, n_trees, rounds = pl.tree()
        assert len(row) == len(col) == len(kin) == 0 and n_trees == 1 and rounds == 0
        assert row.dtype == np.int32 and kin.dtype == np.float32
    finally:
        pl.close()
