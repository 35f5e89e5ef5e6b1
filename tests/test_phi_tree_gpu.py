"""genphi_result_tree, PhiPlan.tree and gen.phiTree on the GPU against tests/phi_tree_oracle.py (Kruskal over the sorted pairs) on the host
matrix of the same plan, shape for shape with tests/test_phi_clusters_gpu.py.  The forest is unique under the strict order of the
edges, so every check is np.array_equal, kinships as bit patterns: no tolerance anywhere."""
import ctypes
import math

import numpy as np
import pytest

import phi_over_oracle as PO
import phi_tree_oracle as TO

pytestmark = pytest.mark.gpu

I32P, F32P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)


def _check(gen, pl, phi, floor, cuts=0, seed=0):
    """The tree of the plan's resident result at `floor` is the oracle's on host matrix phi; its rounds are the host restatement's;
    `cuts` thresholds drawn from the distinct kinships >= floor give genphi_result_clusters' labels and counts.  Returns the tuple
    PhiPlan.tree returns."""
    n = len(phi)
    got = pl.tree(floor)
    row, col, kin, n_trees, rounds = got
    want = TO.forest(phi, floor)
    host = gen._capi.tree_host(phi, floor)
    print("N %d, floor %r: %d edges (oracle %d), %d trees, %d rounds (host %d)" % (n, floor, len(row), len(want[0]), n_trees, rounds, host[4]))
    assert TO.same(got, want) and n_trees == want[3] == n - len(row)
    assert TO.same(host, want)
    assert rounds == host[4] and rounds <= TO.log2_ceil(n) + 1                   # invariant 5
    if cuts and n >= 2:
        f = TO.floor_of(floor)
        distinct = np.unique(phi[np.triu_indices(n, 1)])
        distinct = distinct[distinct.astype(np.float64) >= f]
        if len(distinct):
            tree = gen.PhiTree(f, None, n, row, col, kin, n_trees, rounds)
            for t in np.random.default_rng([20261021, seed, n]).choice(distinct, size=cuts).tolist():
                label = pl.clusters(t)[0]
                k = int(np.count_nonzero(kin.astype(np.float64) >= t))
                assert np.array_equal(tree.cut(t), label)                        # invariant 1
                assert k == n - len(np.unique(label))                            # invariant 2
    return got


# ---- geneaJi ------------------------------------------------------------------------------------------------------------------

def test_geneaJi(gen):
    ped = gen.genealogy(gen.geneaJi)
    assert gen.pro(ped).tolist() == [1, 2, 29]
    phi = gen.phi(ped, device=0)
    top = float(max(phi[0, 1], phi[0, 2], phi[1, 2]))
    above = float(np.nextafter(np.float32(top), np.float32(1)))
    pl = gen.plan(ped)
    try:
        assert np.array_equal(pl.compute(device=0), phi)
        row, col, kin, n_trees, _ = _check(gen, pl, phi, 0.0, cuts=3)
        assert len(row) == 2 and n_trees == 1 and float(kin[0]) == top
        row, col, kin, n_trees, _ = _check(gen, pl, phi, top)
        assert 1 <= len(row) <= 2 and np.all(kin == np.float32(top))
        row, col, kin, n_trees, rounds = _check(gen, pl, phi, above)
        assert len(row) == 0 and n_trees == 3 and rounds == 1
        _check(gen, pl, phi, None)
    finally:
        pl.close()
    for floor in (None, 0.0, top, above):
        want = TO.forest(phi, floor)
        t = gen.phiTree(ped, floor, device=0)
        assert TO.same((t.row, t.col, t.kinship), want) and t.n_trees == want[3] and t.pro.tolist() == [1, 2, 29] and t.rounds >= 1
        assert t.floor == TO.floor_of(floor) and len(t) == len(want[0])
        assert np.array_equal(t.pro1, t.pro[t.row]) and np.array_equal(t.pro2, t.pro[t.col])
        host = gen.phiTree(phi, floor, probandIDs=[1, 2, 29])                      # the host form gives the same answer
        assert TO.same((host.row, host.col, host.kinship), want) and host.n_trees == t.n_trees and host.rounds == 0
        assert np.array_equal(host.pro1, t.pro1) and np.array_equal(host.pro2, t.pro2)
        assert np.array_equal(t.cut(max(TO.floor_of(floor), top)), gen.phiClusters(ped, max(TO.floor_of(floor), top), device=0).label)
    t = gen.phiTree(ped, 0.0, device=0)
    assert "3 probands, 2 edges" in repr(t) and t.linkage().shape == (2, 4) and t.heights()[1][-1] == 1
    c = t.clusters(top)
    ref = gen.phiClusters(ped, top, device=0)
    assert np.array_equal(c.label, ref.label) and np.array_equal(c.sizes, ref.sizes) and np.array_equal(c.pro, ref.pro) and c.n_pairs is None
    # duplicates collapse: positions in [29, 2, 1]
    t = gen.phiTree(ped, 0.0, probandIDs=[29, 2, 29, 1], device=0)
    sub = np.ascontiguousarray(phi[np.ix_([2, 1, 0], [2, 1, 0])])
    assert t.pro.tolist() == [29, 2, 1] and TO.same((t.row, t.col, t.kinship), TO.forest(sub, 0.0))
    with pytest.raises(KeyError):
        gen.phiTree(ped, 0.0, probandIDs=[1, 12345], device=0)
    with pytest.raises(ValueError, match="NaN"):
        gen.phiTree(ped, math.nan, device=0)


# ---- the 2,500 probands of test_phi_clusters_gpu.py --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def synth_case(gen):
    """(pedigree, proband IDs, plan with the full result resident, host matrix).  2,500 probands: ld = 2,560, so 60 zero padding
    columns that a floor <= 0 must not join."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(30_000, 2_500, 10, skip_permille=50)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    phi = pl.compute(device=0)
    assert phi.shape == (2500, 2500) and pl.result_device()[1] == 2560
    yield ped, np.asarray(pro, dtype=np.int64), pl, phi
    pl.close()


@pytest.mark.parametrize("floor", [None, 0.0, -math.inf, math.inf, 1 / 8, 1 / 64, 1 / 1024], ids=["None", "0", "-inf", "+inf", "1/8", "1/64", "1/1024"])
def test_the_2500_probands_against_the_oracle(gen, synth_case, floor):
    _, _, pl, phi = synth_case
    n = len(phi)
    row, col, kin, n_trees, rounds = _check(gen, pl, phi, floor, cuts=6)
    if floor is not None and floor <= 0:
        assert n_trees == 1 and len(row) == n - 1
    elif floor == math.inf:
        assert n_trees == n and len(row) == 0 and rounds == 1
    else:
        assert n_trees == len(np.unique(pl.clusters(TO.floor_of(floor))[0]))


def test_the_function_names_the_probands(gen, synth_case):
    ped, pro, _, phi = synth_case
    want = TO.forest(phi, 1 / 64)
    t = gen.phiTree(ped, 1 / 64, probandIDs=pro, device=0)
    assert TO.same((t.row, t.col, t.kinship), want) and np.array_equal(t.pro, pro) and t.n_trees == want[3]
    assert np.array_equal(t.pro1, pro[want[0]]) and np.array_equal(t.pro2, pro[want[1]])
    assert "%d trees" % want[3] in repr(t) and "2500 probands" in repr(t)
    c, ref = t.clusters(1 / 32), gen.phiClusters(ped, 1 / 32, probandIDs=pro, device=0)
    assert np.array_equal(c.label, ref.label) and np.array_equal(c.cluster, ref.cluster) and np.array_equal(c.sizes, ref.sizes)
    h, left = t.heights()
    assert left[-1] == t.n_trees and np.array_equal(h, np.unique(want[2])[::-1])
    with pytest.raises(ValueError, match="trees"):
        t.linkage()
    z = gen.phiTree(ped, 0.0, probandIDs=pro, device=0).linkage()
    assert z.shape == (2499, 4) and z[-1, 3] == 2500 and np.all(np.diff(z[:, 2]) >= 0)


# ---- sizes at the wave and tile edges ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_sizes_at_the_wave_and_tile_edges(gen, synth_case, n):
    ped, pro, _, _ = synth_case
    pl = gen.plan(ped, pro[:n])
    try:
        phi = pl.compute(device=0)
        assert phi.shape == (n, n)
        t = float(np.median(phi[np.triu_indices(n, 1)])) if n >= 2 else 0.0
        row, col, kin, n_trees, rounds = _check(gen, pl, phi, t, cuts=2)
        if n == 1:
            assert len(row) == 0 and n_trees == 1 and rounds == 0
        _check(gen, pl, phi, 0.0, cuts=2)
    finally:
        pl.close()


# ---- a path, a ring, a star: ties everywhere ------------------------------------------------------------------------------------

def _chain_pedigree(gen, order, ring):
    """301 founders F_0 .. F_300 (IDs 1 .. 301; even ones men, odd ones women) and 300 probands p_k (ID 1001 + k), the child of F_k and
    F_(k + 1): neighbours are half sibs.  ring: p_299 is the child of F_299 and F_0 instead, which makes p_299 and p_0 half sibs too
    (F_299 is a woman, F_0 a man).  The probands listed in `order`."""
    f = np.arange(301)
    k = np.arange(300)
    ind = np.concatenate([1 + f, 1001 + k])
    even_parent, odd_parent = 1 + k + (k % 2), 1 + k + 1 - (k % 2)              # of F_k, F_(k + 1): the even one is the father
    if ring:
        even_parent[299] = 1                                                     # F_0; the mother stays F_299
    father = np.concatenate([np.zeros(301, dtype=np.int64), even_parent])
    mother = np.concatenate([np.zeros(301, dtype=np.int64), odd_parent])
    sex = np.concatenate([1 + (f % 2), 1 + (k % 2)])
    ped = gen.genealogy({"ind": ind, "father": father, "mother": mother, "sex": sex})
    return ped, 1001 + np.asarray(order)


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("ring", [False, True])
def test_a_path_and_a_ring_of_half_sibs(gen, shuffled, ring):
    order = np.random.default_rng(301).permutation(300) if shuffled else np.arange(300)
    ped, pro = _chain_pedigree(gen, order, ring)
    pl = gen.plan(ped, pro)
    try:
        phi = pl.compute(device=0)
        gap = np.abs(order[:, None] - order[None, :])
        want = np.where((gap == 1) | ((gap == 299) & ring), np.float32(0.125), np.float32(0))
        np.fill_diagonal(want, 0.5)
        assert np.array_equal(phi, want.astype(np.float32))                      # half sibs beside each other, strangers otherwise
        for floor in (0.125, None):
            row, col, kin, n_trees, _ = _check(gen, pl, phi, floor)
            assert len(row) == 299 and n_trees == 1 and np.all(kin == np.float32(0.125))
            assert len(set(zip(row.tolist(), col.tolist()))) == 299              # none twice
            assert not TO.labels_of(300, row, col).any()                         # and no cycle: 299 edges that join all 300
        row, col, kin, n_trees, rounds = _check(gen, pl, phi, float(np.nextafter(0.125, math.inf)))
        assert len(row) == 0 and n_trees == 300 and rounds == 1
        row, col, kin, n_trees, _ = _check(gen, pl, phi, 0.0)
        assert len(row) == 299 and np.all(kin == np.float32(0.125))
    finally:
        pl.close()


def test_200_full_sibs_give_the_star_at_position_0(gen):
    ind = np.arange(1, 203)
    father = np.concatenate([[0, 0], np.full(200, 1)])
    mother = np.concatenate([[0, 0], np.full(200, 2)])
    sex = np.concatenate([[1, 2], 1 + np.arange(200) % 2])
    ped = gen.genealogy({"ind": ind, "father": father, "mother": mother, "sex": sex})
    pl = gen.plan(ped, ind[2:])
    try:
        phi = pl.compute(device=0)
        assert np.all(phi[np.triu_indices(200, 1)] == np.float32(0.25))
        for floor in (None, 0.0, 0.25):
            row, col, kin, n_trees, rounds = _check(gen, pl, phi, floor)
            assert row.tolist() == [0] * 199 and col.tolist() == list(range(1, 200)) and n_trees == 1 and rounds == 1
    finally:
        pl.close()


# ---- the contract -------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_outputs_and_the_plan_alone(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(4000, 400, 10, skip_permille=50)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    L, C = gen._capi.lib(), gen._capi
    n = pl.n_probands

    def c_call(floor, code):
        """The entry point returns `code` at `floor` and leaves its outputs as they were."""
        row, col, kin = np.full(n - 1, -7, np.int32), np.full(n - 1, -7, np.int32), np.full(n - 1, -7, np.float32)
        k, trees, rounds = ctypes.c_int64(-7), ctypes.c_int64(-7), ctypes.c_int32(-7)
        rc = L.genphi_result_tree(pl._h, floor, row.ctypes.data_as(I32P), col.ctypes.data_as(I32P), kin.ctypes.data_as(F32P), ctypes.byref(k),
                                  ctypes.byref(trees), ctypes.byref(rounds))
        assert rc == code
        assert np.all(row == -7) and np.all(col == -7) and np.all(kin == -7) and (k.value, trees.value, rounds.value) == (-7, -7, -7)

    try:
        c_call(0.01, C.GENPHI_ERR_DEVICE)                                        # no resident result yet
        with pytest.raises(gen.GenphiDeviceError):
            pl.tree(0.01)
        phi = pl.compute(device=0)
        distinct = np.unique(phi[np.triu_indices(n, 1)])[::-1]
        t, t2 = float(distinct[len(distinct) // 4]), float(distinct[len(distinct) // 2])
        assert t != t2
        want = TO.forest(phi, t)

        def good():
            assert TO.same(pl.tree(t), want)
            assert np.array_equal(pl.result_to_host(), phi)

        good()
        c_call(math.nan, C.GENPHI_ERR_ARG)
        with pytest.raises(ValueError, match="NaN"):
            pl.tree(math.nan)
        good()
        # any output may be NULL
        assert L.genphi_result_tree(pl._h, t, None, None, None, None, None, None) == 0
        k, trees, rounds = ctypes.c_int64(-7), ctypes.c_int64(-7), ctypes.c_int32(-7)
        assert L.genphi_result_tree(pl._h, t, None, None, None, ctypes.byref(k), None, None) == 0 and k.value == len(want[0])
        assert L.genphi_result_tree(pl._h, t, None, None, None, None, ctypes.byref(trees), ctypes.byref(rounds)) == 0
        assert trees.value == want[3] and rounds.value == gen._capi.tree_host(phi, t)[4]
        col = np.full(n - 1, -7, np.int32)
        assert L.genphi_result_tree(pl._h, t, None, col.ctypes.data_as(I32P), None, None, None, None) == 0
        assert np.array_equal(col[:len(want[1])], want[1]) and np.all(col[len(want[1]):] == -7)      # entries from M on are not written
        for rows in ((0, 100), (100, n), (0, n - 1), (5, 5)):                    # a row shard, an empty one too
            pl.compute_device(device=0, rows=rows)
            c_call(t, C.GENPHI_ERR_ARG)
            with pytest.raises(ValueError, match="rows are resident"):
                pl.tree(t)
        pl.compute_device(device=0)
        good()
        pl.compute_device(device=0, storage64=True)                              # a Float64 result
        c_call(t, C.GENPHI_ERR_ARG)
        with pytest.raises(ValueError, match="Float32"):
            pl.tree(t)
        pl.compute_device(device=0)
        good()
        pl.release_device()
        c_call(t, C.GENPHI_ERR_DEVICE)
        pl.compute_device(device=0)
        good()
        # the counts phiOver keeps, and the scratch block the queries share: a count at t, the tree at another floor, then the list at t
        ref = PO.over_numpy(phi, t)
        assert pl.count_over(t) == len(ref[0])
        assert TO.same(pl.tree(t2), TO.forest(phi, t2))
        assert PO.same(pl.phi_over(t), ref) and pl.count_over(t) == len(ref[0])
        assert TO.same(pl.tree(t2), TO.forest(phi, t2))
        assert PO.same(pl.phi_over(t), ref)
    finally:
        pl.close()


def test_the_same_call_gives_the_same_bytes(synth_case):
    _, _, pl, _ = synth_case
    for floor in (1 / 64, 0.0, None):
        a, b = pl.tree(floor), pl.tree(floor)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:]
