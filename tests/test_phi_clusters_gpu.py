"""genphi_result_clusters / genphi_result_unrelated, PhiPlan.clusters / PhiPlan.unrelated, gen.phiClusters / gen.phiUnrelated on the
GPU against tests/phi_clusters_oracle.py, on the host matrix of the same plan.  The queries only compare and count, so every check is
np.array_equal: no tolerance anywhere."""
import ctypes
import math

import numpy as np
import pytest

import phi_clusters_oracle as CO
import phi_over_oracle as PO

pytestmark = pytest.mark.gpu

I32P, U8P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8)


def _tie_priority(n, seed=20261020):
    """A seeded int32 priority array with many ties, negative values and the ends of the range."""
    r = np.random.default_rng([seed, n])
    pri = r.integers(-4, 5, n).astype(np.int32)
    if n >= 8:
        pri[r.integers(n)] = np.iinfo(np.int32).min
        pri[r.integers(n)] = np.iinfo(np.int32).max
    return pri


def _check(pl, phi, t):
    """Both queries of the plan's resident result at threshold t are the oracle's on host matrix phi; returns (label, keep by
    degree, rounds by degree)."""
    a = CO.adjacency(phi, t)
    n = len(phi)
    label, pairs = pl.clusters(t)
    assert label.dtype == np.int32 and np.array_equal(label, CO.components(a))
    assert pairs == CO.n_pairs(a) == pl.count_over(t)
    deg = CO.degrees(a)
    out = None
    for name, pri in (("degree", None), ("position", np.zeros(n, dtype=np.int32)), ("ties", _tie_priority(n))):
        keep, degree, rounds = pl.unrelated(t, pri)
        ref = CO.greedy(a, pri)
        jac, ref2 = CO.jacobi_rounds(a, CO.keys(a, pri))
        print("N %d, threshold %r, %s: %d pairs, %d kept (oracle %d), %d rounds (synchronous %d)" % (
            n, t, name, CO.n_pairs(a), int(keep.sum()), int(ref.sum()), rounds, jac))
        assert np.array_equal(ref, ref2)
        assert keep.dtype == bool and np.array_equal(keep, ref)
        assert degree.dtype == np.int32 and np.array_equal(degree, deg)
        assert CO.is_independent(a, keep) and CO.is_maximal(a, keep)
        assert (1 if n >= 2 else 0) <= rounds <= jac
        if out is None:
            out = (label, keep, rounds)
    return out


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
        label, keep, _ = _check(pl, phi, 0.0)
        assert label.tolist() == [0, 0, 0] and keep.tolist() == [True, False, False]
        label, keep, _ = _check(pl, phi, top)
        assert len(set(label.tolist())) < 3 and not keep.all()
        label, keep, _ = _check(pl, phi, above)
        assert label.tolist() == [0, 1, 2] and keep.all()
    finally:
        pl.close()
    for t in (0.0, top, above):
        a = CO.adjacency(phi, t)
        c = gen.phiClusters(ped, t, device=0)
        assert np.array_equal(c.label, CO.components(a)) and c.n_pairs == CO.n_pairs(a) and c.pro.tolist() == [1, 2, 29]
        host = gen.phiClusters(phi, t, probandIDs=[1, 2, 29])                  # the host form gives the same answer
        assert np.array_equal(host.label, c.label) and np.array_equal(host.cluster, c.cluster) and np.array_equal(host.sizes, c.sizes)
        assert host.n_pairs == c.n_pairs and np.array_equal(host.pro, c.pro)
        assert [c.members(k).tolist() for k in range(len(c))] == [host.members(k).tolist() for k in range(len(c))]
        for pri in (None, "degree", "position", [5, -5, 5]):
            u = gen.phiUnrelated(ped, t, priority=pri, device=0)
            h = gen.phiUnrelated(phi, t, priority=pri, probandIDs=[1, 2, 29])
            assert np.array_equal(u.keep, CO.greedy(a, None if pri in (None, "degree") else np.zeros(3) if pri == "position" else pri))
            assert np.array_equal(u.keep, h.keep) and np.array_equal(u.index, h.index) and np.array_equal(u.kept, h.kept)
            assert np.array_equal(u.degree, h.degree) and u.rounds >= 1 and h.rounds == 0
    c = gen.phiClusters(ped, 0.0, device=0)
    assert "1 clusters" in repr(c) and c.members(0).tolist() == [1, 2, 29] and c.sizes.tolist() == [3]
    # duplicates collapse: positions in [29, 2, 1]
    c = gen.phiClusters(ped, top, probandIDs=[29, 2, 29, 1], device=0)
    sub = phi[np.ix_([2, 1, 0], [2, 1, 0])]
    assert c.pro.tolist() == [29, 2, 1] and np.array_equal(c.label, CO.components(CO.adjacency(sub, top)))
    u = gen.phiUnrelated(ped, top, priority="position", probandIDs=[29, 2, 29, 1], device=0)
    ref = CO.greedy(CO.adjacency(sub, top), np.zeros(3))
    assert u.pro.tolist() == [29, 2, 1] and np.array_equal(u.keep, ref) and u.kept.tolist() == np.array([29, 2, 1])[ref].tolist()
    assert "of 3 probands kept" in repr(u)
    with pytest.raises(KeyError):
        gen.phiClusters(ped, 0.0, probandIDs=[1, 12345], device=0)
    with pytest.raises(KeyError):
        gen.phiUnrelated(ped, 0.0, probandIDs=[1, 12345], device=0)
    with pytest.raises(ValueError):
        gen.phiUnrelated(ped, 0.0, priority=[1, 2], device=0)                  # wrong length


# ---- the 2,500 probands of test_phi_over_gpu.py -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def synth_case(gen):
    """(pedigree, proband IDs, plan with the full result resident, host matrix).  2,500 probands: ld = 2,560, so 60 zero padding
    columns that a threshold <= 0 must not join."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(30_000, 2_500, 10, skip_permille=50)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    phi = pl.compute(device=0)
    assert phi.shape == (2500, 2500) and pl.result_device()[1] == 2560
    yield ped, np.asarray(pro, dtype=np.int64), pl, phi
    pl.close()


@pytest.mark.parametrize("t", [-math.inf, 0.0, math.inf, 1 / 8, 1 / 64, 1 / 1024], ids=["-inf", "0", "+inf", "1/8", "1/64", "1/1024"])
def test_the_2500_probands_against_the_oracle(synth_case, t):
    _, _, pl, phi = synth_case
    n = len(phi)
    label, keep, rounds = _check(pl, phi, t)
    a = phi.astype(np.float64) >= t                                            # independence and maximality on the host matrix itself
    np.fill_diagonal(a, False)
    assert not a[np.ix_(keep, keep)].any() and np.all(keep | a[:, keep].any(axis=1))
    if t <= 0:
        assert not label.any() and keep.tolist() == [True] + [False] * (n - 1)
        assert np.all(pl.unrelated(t)[1] == n - 1) and pl.clusters(t)[1] == n * (n - 1) // 2
    elif t == math.inf:
        assert np.array_equal(label, np.arange(n)) and keep.all() and not pl.unrelated(t)[1].any() and pl.clusters(t)[1] == 0
    else:
        assert 1 < len(np.unique(label)) < n and 1 < int(keep.sum()) < n


def test_the_functions_name_the_probands(gen, synth_case):
    ped, pro, _, phi = synth_case
    t = 1 / 64
    a = CO.adjacency(phi, t)
    c = gen.phiClusters(ped, t, probandIDs=pro, device=0)
    label = CO.components(a)
    assert np.array_equal(c.label, label) and np.array_equal(c.pro, pro) and c.n_pairs == CO.n_pairs(a)
    firsts = np.flatnonzero(label == np.arange(len(label)))
    assert len(c) == len(firsts) and np.array_equal(c.sizes, [np.count_nonzero(label == f) for f in firsts])
    k = int(np.argmax(c.sizes))
    assert np.array_equal(c.members(k), pro[label == firsts[k]]) and np.array_equal(c.cluster == k, label == firsts[k])
    assert "%d clusters" % len(firsts) in repr(c) and "largest of %d" % c.sizes.max() in repr(c)
    host = gen.phiClusters(phi, t, probandIDs=pro)
    assert np.array_equal(host.label, c.label) and np.array_equal(host.cluster, c.cluster) and host.n_pairs == c.n_pairs
    pri = _tie_priority(len(phi))
    for p, ref_pri in (("degree", None), ("position", np.zeros(len(phi))), (pri, pri)):
        u = gen.phiUnrelated(ped, t, priority=p, probandIDs=pro, device=0)
        ref = CO.greedy(a, ref_pri)
        assert np.array_equal(u.keep, ref) and np.array_equal(u.index, np.flatnonzero(ref)) and np.array_equal(u.kept, pro[ref])
        assert np.array_equal(u.degree, CO.degrees(a))
        h = gen.phiUnrelated(phi, t, priority=p, probandIDs=pro)
        assert np.array_equal(h.keep, u.keep) and np.array_equal(h.degree, u.degree) and np.array_equal(h.kept, u.kept)


# ---- sizes at the wave and tile edges ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_sizes_at_the_wave_and_tile_edges(gen, synth_case, n):
    ped, pro, _, _ = synth_case
    pl = gen.plan(ped, pro[:n])
    try:
        phi = pl.compute(device=0)
        assert phi.shape == (n, n)
        t = float(np.median(phi[np.triu_indices(n, 1)])) if n >= 2 else 0.0
        label, keep, _ = _check(pl, phi, t)
        if n == 1:
            assert label.tolist() == [0] and keep.tolist() == [True]
        _check(pl, phi, 0.0)
    finally:
        pl.close()


# ---- a path: the worst case of both kernels -------------------------------------------------------------------------------------

def _path_pedigree(gen, order):
    """301 founders F_0 .. F_300 (IDs 1 .. 301; even ones men, odd ones women) and 300 probands p_k (ID 1001 + k), the child of F_k and
    F_(k + 1): neighbours are half sibs.  The probands listed in `order`."""
    f = np.arange(301)
    k = np.arange(300)
    ind = np.concatenate([1 + f, 1001 + k])
    even_parent, odd_parent = 1 + k + (k % 2), 1 + k + 1 - (k % 2)              # of F_k, F_(k + 1): the even one is the father
    father = np.concatenate([np.zeros(301, dtype=np.int64), even_parent])
    mother = np.concatenate([np.zeros(301, dtype=np.int64), odd_parent])
    sex = np.concatenate([1 + (f % 2), 1 + (k % 2)])
    ped = gen.genealogy({"ind": ind, "father": father, "mother": mother, "sex": sex})
    return ped, 1001 + np.asarray(order)


@pytest.mark.parametrize("shuffled", [False, True])
def test_a_path_graph(gen, shuffled):
    order = np.random.default_rng(301).permutation(300) if shuffled else np.arange(300)
    ped, pro = _path_pedigree(gen, order)
    pl = gen.plan(ped, pro)
    try:
        phi = pl.compute(device=0)
        want = np.where(np.abs(order[:, None] - order[None, :]) == 1, np.float32(0.125), np.float32(0))
        np.fill_diagonal(want, 0.5)
        assert np.array_equal(phi, want.astype(np.float32))                      # half sibs beside each other, strangers otherwise
        a = CO.adjacency(phi, 0.125)
        label, pairs = pl.clusters(0.125)
        assert not label.any() and pairs == 299 and np.array_equal(label, CO.components(a))
        for name, pri in (("position", np.zeros(300, dtype=np.int32)), ("degree", None)):
            keep, degree, rounds = pl.unrelated(0.125, pri)
            jac, ref = CO.jacobi_rounds(a, CO.keys(a, pri))
            print("path, shuffled %s, by %s: %d kept, %d rounds (synchronous %d)" % (shuffled, name, int(keep.sum()), rounds, jac))
            assert np.array_equal(keep, CO.greedy(a, pri)) and np.array_equal(keep, ref) and np.array_equal(degree, CO.degrees(a))
            assert 1 <= rounds <= jac
            if not shuffled and name == "position":
                assert np.array_equal(keep, np.arange(300) % 2 == 0)
        step = float(np.nextafter(0.125, math.inf))
        label, pairs = pl.clusters(step)
        keep, degree, _ = pl.unrelated(step)
        assert np.array_equal(label, np.arange(300)) and pairs == 0 and keep.all() and not degree.any()
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
    pri = _tie_priority(n)

    def c_calls(t, code, member=True):
        """Both entry points (member=False: genphi_result_unrelated without its member array) return `code` at threshold t and
        leave their outputs as they were."""
        if member:
            label, k, pairs = np.full(n, -7, np.int32), ctypes.c_int64(-7), ctypes.c_int64(-7)
            assert L.genphi_result_clusters(pl._h, t, label.ctypes.data_as(I32P), ctypes.byref(k), ctypes.byref(pairs)) == code
            assert np.all(label == -7) and k.value == -7 and pairs.value == -7
        for p in (None, pri):
            mem, deg, kept, rounds = np.full(n, 7, np.uint8), np.full(n, -7, np.int32), ctypes.c_int64(-7), ctypes.c_int32(-7)
            rc = L.genphi_result_unrelated(pl._h, t, None if p is None else p.ctypes.data_as(I32P), mem.ctypes.data_as(U8P) if member else None,
                                           deg.ctypes.data_as(I32P), ctypes.byref(kept), ctypes.byref(rounds))
            assert rc == code
            assert np.all(mem == 7) and np.all(deg == -7) and kept.value == -7 and rounds.value == -7

    try:
        c_calls(0.01, C.GENPHI_ERR_DEVICE)                                       # no resident result yet
        with pytest.raises(gen.GenphiDeviceError):
            pl.clusters(0.01)
        with pytest.raises(gen.GenphiDeviceError):
            pl.unrelated(0.01)
        phi = pl.compute(device=0)
        distinct = np.unique(phi[np.triu_indices(n, 1)])[::-1]
        t, t2 = float(distinct[len(distinct) // 4]), float(distinct[len(distinct) // 2])
        assert t != t2

        def good():
            _check(pl, phi, t)
            assert np.array_equal(pl.result_to_host(), phi)

        good()
        c_calls(math.nan, C.GENPHI_ERR_ARG)
        for call in (lambda: pl.clusters(math.nan), lambda: pl.unrelated(math.nan)):
            with pytest.raises(ValueError):
                call()
        good()
        c_calls(t, C.GENPHI_ERR_ARG, member=False)                               # NULL member
        good()
        # any other output may be NULL
        assert L.genphi_result_clusters(pl._h, t, None, None, None) == 0
        mem = np.full(n, 7, np.uint8)
        assert L.genphi_result_unrelated(pl._h, t, None, mem.ctypes.data_as(U8P), None, None, None) == 0
        assert np.array_equal(mem.astype(bool), CO.greedy(CO.adjacency(phi, t)))
        mem = np.full(n, 7, np.uint8)                                            # priorities and no degrees: no degree pass
        assert L.genphi_result_unrelated(pl._h, t, pri.ctypes.data_as(I32P), mem.ctypes.data_as(U8P), None, None, None) == 0
        assert np.array_equal(mem.astype(bool), CO.greedy(CO.adjacency(phi, t), pri))
        k, kept = ctypes.c_int64(-7), ctypes.c_int64(-7)
        assert L.genphi_result_clusters(pl._h, t, None, ctypes.byref(k), None) == 0
        assert k.value == len(np.unique(CO.components(CO.adjacency(phi, t))))
        assert L.genphi_result_unrelated(pl._h, t, None, mem.ctypes.data_as(U8P), None, ctypes.byref(kept), None) == 0
        assert kept.value == int(CO.greedy(CO.adjacency(phi, t)).sum())
        for rows in ((0, 100), (100, n), (0, n - 1), (5, 5)):                    # a row shard, an empty one too
            pl.compute_device(device=0, rows=rows)
            c_calls(t, C.GENPHI_ERR_ARG)
            with pytest.raises(ValueError, match="rows are resident"):
                pl.clusters(t)
            with pytest.raises(ValueError, match="rows are resident"):
                pl.unrelated(t)
        pl.compute_device(device=0)
        good()
        pl.compute_device(device=0, storage64=True)                              # a Float64 result
        c_calls(t, C.GENPHI_ERR_ARG)
        with pytest.raises(ValueError, match="Float32"):
            pl.clusters(t)
        with pytest.raises(ValueError, match="Float32"):
            pl.unrelated(t)
        pl.compute_device(device=0)
        good()
        pl.release_device()
        c_calls(t, C.GENPHI_ERR_DEVICE)
        pl.compute_device(device=0)
        good()
        # the counts phiOver keeps, and the scratch block the queries share: a count at t, the cluster queries at another threshold,
        # then the list at t
        ref = PO.over_numpy(phi, t)
        assert pl.count_over(t) == len(ref[0])
        label, pairs = pl.clusters(t2)
        keep = pl.unrelated(t2)[0]
        assert PO.same(pl.phi_over(t), ref) and pl.count_over(t) == len(ref[0])
        a2 = CO.adjacency(phi, t2)
        assert np.array_equal(label, CO.components(a2)) and pairs == CO.n_pairs(a2) == pl.count_over(t2) and np.array_equal(keep, CO.greedy(a2))
        assert PO.same(pl.phi_over(t), ref)
    finally:
        pl.close()


def test_the_same_call_gives_the_same_bytes(synth_case):
    _, _, pl, phi = synth_case
    pri = _tie_priority(len(phi))
    for t in (1 / 64, 0.0):
        a, b = pl.clusters(t), pl.clusters(t)
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
        for p in (None, pri):
            a, b = pl.unrelated(t, p), pl.unrelated(t, p)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
