"""gen.phiClusters / gen.phiUnrelated on a square host matrix (no GPU): numpy and a plain loop in the package, against
tests/phi_clusters_oracle.py on small hand-made matrices.  Every comparison is np.array_equal."""
import math

import numpy as np
import pytest

import phi_clusters_oracle as CO


def _matrix(n, edges, value=0.125, diag=0.5):
    m = np.zeros((n, n), dtype=np.float32)
    for i, j in edges:
        m[i, j] = m[j, i] = value
    np.fill_diagonal(m, diag)
    return m


# two triangles 0-1-2 and 3-4-5 joined by the edge 2-3, an isolated vertex 6, a pair 7-8
EDGES = [(0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5), (2, 3), (7, 8)]


def _check(gen, m, t, ids=None):
    a = CO.adjacency(m, t)
    c = gen.phiClusters(m, t, probandIDs=ids)
    assert c.label.dtype == np.int32 and np.array_equal(c.label, CO.components(a)) and c.n_pairs == CO.n_pairs(a)
    out = [c]
    n = len(m)
    tie = np.arange(n) % 2                                                       # ties in priority: the position decides
    for name, pri in (("degree", None), ("position", np.zeros(n, dtype=np.int64)), (tie, tie), (None, None)):
        u = gen.phiUnrelated(m, t, priority=name, probandIDs=ids)
        ref = CO.greedy(a, pri)
        assert u.keep.dtype == bool and np.array_equal(u.keep, ref) and np.array_equal(u.degree, CO.degrees(a))
        assert u.degree.dtype == np.int32 and u.index.dtype == np.int32 and np.array_equal(u.index, np.flatnonzero(ref))
        assert CO.is_independent(a, u.keep) and CO.is_maximal(a, u.keep)
        assert np.array_equal(CO.jacobi_rounds(a, CO.keys(a, pri))[1], ref)      # (the oracle's two forms agree)
        out.append(u)
    return out


def test_two_triangles_joined_by_one_edge_and_an_isolated_vertex(gen):
    m = _matrix(9, EDGES)
    c, by_degree, by_position, by_tie, default = _check(gen, m, 0.125)
    assert c.label.tolist() == [0, 0, 0, 0, 0, 0, 6, 7, 7] and c.n_pairs == 8
    assert c.cluster.tolist() == [0, 0, 0, 0, 0, 0, 1, 2, 2] and c.cluster.dtype == np.int32
    assert c.sizes.tolist() == [6, 1, 2] and c.sizes.dtype == np.int64 and len(c) == 3
    assert c.members(0).tolist() == [0, 1, 2, 3, 4, 5] and c.members(1).tolist() == [6] and c.members(2).tolist() == [7, 8]
    with pytest.raises(IndexError):
        c.members(3)
    assert "3 clusters" in repr(c) and "largest of 6" in repr(c)
    assert c.pro is None and by_degree.pro is None and by_degree.kept is None
    # degrees 2 2 3 3 2 2 0 1 1: vertex 6 first, then 7 (bars 8), then 0 (bars 1, 2), then 4 (bars 3, 5)
    assert by_degree.degree.tolist() == [2, 2, 3, 3, 2, 2, 0, 1, 1]
    assert by_degree.index.tolist() == [0, 4, 6, 7] and np.array_equal(default.keep, by_degree.keep)
    # by position: 0 (bars 1, 2), 3 (bars 4, 5), 6, 7
    assert by_position.index.tolist() == [0, 3, 6, 7]
    # priorities 0 1 0 1 ...: the even positions first, in order: 0 (bars 1, 2), 4 (bars 3, 5), 6, 8 (bars 7)
    assert by_tie.index.tolist() == [0, 4, 6, 8]
    assert "4 of 9 probands kept" in repr(by_degree) and len(by_degree) == 4 and by_degree.rounds == 0


def test_ids_name_the_members(gen):
    m = _matrix(9, EDGES)
    ids = np.array([90, 80, 70, 60, 50, 40, 30, 20, 10])
    c, by_degree = _check(gen, m, 0.125, ids=ids)[:2]
    assert np.array_equal(c.pro, ids) and c.members(2).tolist() == [20, 10] and c.members(1).tolist() == [30]
    assert by_degree.kept.tolist() == [90, 50, 30, 20] and np.array_equal(by_degree.pro, ids)


def test_thresholds_at_the_ends(gen):
    m = _matrix(9, EDGES)
    for t in (0.0, -1.0, -math.inf):                                             # every pair is an edge: zeros are >= 0
        c, by_degree, by_position = _check(gen, m, t)[:3]
        assert c.label.tolist() == [0] * 9 and c.n_pairs == 36 and c.sizes.tolist() == [9]
        assert by_degree.index.tolist() == [0] and by_position.index.tolist() == [0] and by_degree.degree.tolist() == [8] * 9
    for t in (math.inf, 0.126, 1.0):                                             # (the diagonal's 0.5 is never an edge)
        c, by_degree = _check(gen, m, t)[:2]
        assert c.label.tolist() == list(range(9)) and c.n_pairs == 0 and c.sizes.tolist() == [1] * 9
        assert by_degree.keep.all() and not by_degree.degree.any()


def test_a_threshold_between_two_float32_values(gen):
    """Entries at 0.1f and at the next Float32 above it; thresholds at either value and one Float64 step above the lower one: the
    comparison is float64(entry) >= threshold."""
    lo = np.float32(0.1)
    hi = np.nextafter(lo, np.float32(1))
    m = _matrix(5, [(0, 1), (1, 2)], value=lo)
    m[3, 4] = m[4, 3] = hi
    c = _check(gen, m, float(lo))[0]
    assert c.label.tolist() == [0, 0, 0, 3, 3] and c.n_pairs == 3
    between = float(np.nextafter(np.float64(lo), np.inf))                        # above float64(lo), below float64(hi)
    assert float(lo) < between < float(hi)
    c, u = _check(gen, m, between)[:2]
    assert c.label.tolist() == [0, 1, 2, 3, 3] and c.n_pairs == 1 and u.index.tolist() == [0, 1, 2, 3]
    assert _check(gen, m, 0.1)[0].n_pairs == 3                                   # the double 0.1 lies below float64(0.1f)
    assert _check(gen, m, float(np.nextafter(np.float64(hi), np.inf)))[0].n_pairs == 0


def test_small_matrices(gen):
    for n in (0, 1, 2):
        m = np.full((n, n), 0.25, dtype=np.float32)
        c = gen.phiClusters(m, 0.25)
        u = gen.phiUnrelated(m, 0.25)
        assert c.label.tolist() == [0] * n and c.n_pairs == n * (n - 1) // 2 and len(c) == min(n, 1)
        assert u.keep.tolist() == [True, False][:n] and u.degree.tolist() == [n - 1] * n
        assert repr(c) and repr(u)


def test_a_random_matrix_with_many_ties(gen):
    rng = np.random.default_rng(20261020)
    n = 60
    m = rng.choice(np.array([0, 0, 0, 0, 2.0 ** -6, 2.0 ** -4, 2.0 ** -3], dtype=np.float32), size=(n, n))
    m = np.triu(m, 1)
    m = (m + m.T).astype(np.float32)
    np.fill_diagonal(m, 0.5)
    pri = rng.integers(-3, 3, n)
    for t in (2.0 ** -3, 2.0 ** -4, 2.0 ** -6, 0.0):
        a = CO.adjacency(m, t)
        _check(gen, m, t)
        u = gen.phiUnrelated(m, t, priority=pri)
        assert np.array_equal(u.keep, CO.greedy(a, pri))
        u = gen.phiUnrelated(m, t, priority=pri.tolist())
        assert np.array_equal(u.keep, CO.greedy(a, pri))


def test_value_errors(gen):
    m = _matrix(9, EDGES)
    for fn in (gen.phiClusters, gen.phiUnrelated):
        with pytest.raises(ValueError, match="NaN"):
            fn(m, math.nan)
        with pytest.raises(ValueError, match="square"):
            fn(m[:, :8], 0.125)
        with pytest.raises(ValueError, match="square"):
            fn(m[0], 0.125)
        with pytest.raises(ValueError, match="probandIDs"):
            fn(m, 0.125, probandIDs=np.arange(8))
    with pytest.raises(ValueError, match="priority"):
        gen.phiUnrelated(m, 0.125, priority=np.arange(8))                        # wrong length
    with pytest.raises(ValueError, match="priority"):
        gen.phiUnrelated(m, 0.125, priority=np.zeros((9, 1), dtype=np.int64))
    with pytest.raises(ValueError, match="integers"):
        gen.phiUnrelated(m, 0.125, priority=np.linspace(0.0, 1.0, 9))            # not integers
    with pytest.raises(ValueError, match="int32"):
        gen.phiUnrelated(m, 0.125, priority=np.arange(9, dtype=np.int64) << 32)
    with pytest.raises(ValueError, match="priority"):
        gen.phiUnrelated(m, 0.125, priority="random")


def test_the_plan_has_the_methods_and_the_library_the_symbols(gen):
    assert callable(gen.PhiPlan.clusters) and callable(gen.PhiPlan.unrelated)
    L = gen._capi.lib()
    assert hasattr(L, "genphi_result_clusters") and hasattr(L, "genphi_result_unrelated")
    ped = gen.genealogy(gen.geneaJi)
    pl = gen.plan(ped)
    try:
        for call in (lambda: pl.clusters(math.nan), lambda: pl.unrelated(math.nan)):
            with pytest.raises(ValueError, match="NaN"):
                call()
        with pytest.raises(gen.GenphiDeviceError):                               # never computed: no resident result
            pl.clusters(0.1)
        with pytest.raises(gen.GenphiDeviceError):
            pl.unrelated(0.1)
    finally:
        pl.close()
    pl = gen.plan(ped, [29])                                                     # one proband: the trivial answer, no device needed
    try:
        label, pairs = pl.clusters(0.0)
        keep, degree, rounds = pl.unrelated(0.0)
        assert label.tolist() == [0] and pairs == 0 and keep.tolist() == [True] and degree.tolist() == [0] and rounds == 0
    finally:
        pl.close()
