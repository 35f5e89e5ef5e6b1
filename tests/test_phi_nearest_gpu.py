"""genphi_result_nearest / PhiPlan.nearest / gen.phiNearest on the GPU against tests/phi_nearest_oracle.py, on the host matrix of
the same plan (or the committed oracle matrix).  The selection only compares and copies, so every check is np.array_equal (values
as bit patterns): no tolerance anywhere."""
import ctypes
import os

import numpy as np
import pytest

import phi_nearest_oracle as PN
from test_phi_over_gpu import synth_case                    # noqa: F401  (the 2,500 probands of the phiOver tests: a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN140 = os.path.join(ROOT, "tests", "golden", "genea140_phi_oracle.npy")
TILE = 4096                                                  # columns a workgroup of nearest_kernel takes between two barriers


def _check(pl, phi_rows, k, row_begin=0, rows=None):
    """nearest(k) of the plan's resident rows (phi_rows = those rows on the host) is the oracle's answer; returns it.  rows: check
    only these resident rows against the oracle (a slice; large matrices), the shape and the candidates' range always."""
    cols, vals = pl.nearest(k)
    n = phi_rows.shape[1]
    assert cols.shape == vals.shape == (len(phi_rows), k) and cols.dtype == np.int32 and vals.dtype == np.float32
    assert cols.min() >= 0 and cols.max() < n                                   # never a padding column
    assert not np.any(cols == (row_begin + np.arange(len(phi_rows)))[:, None])  # never the diagonal
    sl = slice(None) if rows is None else rows
    first = row_begin + (sl.start or 0)
    assert PN.same((cols[sl], vals[sl]), PN.nearest_numpy(phi_rows[sl], k, row_begin=first))
    return cols, vals


# ---- geneaJi ------------------------------------------------------------------------------------------------------------------

def test_geneaJi_known_answer(gen):
    ped = gen.genealogy(gen.geneaJi)
    index = [[1, 2], [0, 2], [0, 1]]                                            # row 2 is the tie: decided by column
    kinship = [[0.37109375, 0.072265625], [0.37109375, 0.072265625], [0.072265625, 0.072265625]]
    pl = gen.plan(ped)
    try:
        phi = pl.compute(device=0)
        cols, vals = _check(pl, phi, 2)
        assert cols.tolist() == index and vals.tolist() == kinship
        assert PN.same((cols, vals), PN.nearest_literal(phi, 2))
        assert pl.nearest(1)[0].tolist() == [[1], [0], [0]]
    finally:
        pl.close()
    got = gen.phiNearest(ped, k=2, device=0)
    assert got.index.tolist() == index and got.kinship.tolist() == kinship and got.k == 2
    assert got.pro.tolist() == [1, 2, 29] and got.relative.tolist() == [[2, 29], [1, 29], [1, 2]]
    assert gen.phiNearest(ped, device=0).k == 2                                 # k = 10 clipped to N - 1
    got = gen.phiNearest(ped, 1, probandIDs=[29, 2, 29, 1], device=0)           # duplicates collapse: positions in [29, 2, 1]
    assert got.pro.tolist() == [29, 2, 1] and got.index.tolist() == [[1], [2], [1]] and got.relative.tolist() == [[2], [1], [2]]
    assert "nearest relatives of 3 probands" in repr(got)


# ---- the 2,500 probands of test_phi_over_gpu.py -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def synth_ref(synth_case):
    """The oracle's answer at k = 64, computed once; its first k columns are its answer at k (one sort, cut at k)."""
    phi = synth_case[3]
    ref = PN.nearest_numpy(phi, 64)
    assert PN.same(tuple(a[:40, :10] for a in ref), PN.nearest_literal(phi[:40], 10))
    return ref


@pytest.mark.parametrize("k", [1, 2, 10, 63, 64])
def test_synthetic_case(synth_case, synth_ref, k):
    _, _, pl, phi, _ = synth_case
    cols, vals = pl.nearest(k)
    assert PN.same((cols, vals), tuple(np.ascontiguousarray(a[:, :k]) for a in synth_ref))
    assert cols.max() < 2500 and not np.any(cols == np.arange(2500)[:, None])   # ld = 2,560: 60 padding columns of zeros
    assert pl.stats.nearest_buf == 1024                                         # the default buffer


def test_cols_only_and_values_only(gen, synth_case, synth_ref):
    _, _, pl, phi, _ = synth_case
    c, v = pl.nearest(10, values=False)
    assert v is None and np.array_equal(c, synth_ref[0][:, :10])
    c, v = pl.nearest(10, cols=False)
    assert c is None and v.tobytes() == np.ascontiguousarray(synth_ref[1][:, :10]).tobytes()
    L = gen._capi.lib()                                                         # the array not asked for is not touched
    cols = np.full((2500, 3), -7, np.int32)
    assert L.genphi_result_nearest(pl._h, 3, cols.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None) == 0
    assert np.array_equal(cols, synth_ref[0][:, :3])
    assert L.genphi_result_nearest(pl._h, 3, None, None) == gen._capi.GENPHI_ERR_ARG


def test_the_same_call_gives_the_same_bytes_and_a_smaller_k_is_a_prefix(synth_case):
    _, _, pl, _, _ = synth_case
    a, b = pl.nearest(64), pl.nearest(64)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    for k in (1, 7, 63):
        c, v = pl.nearest(k)
        assert np.array_equal(c, a[0][:, :k]) and v.tobytes() == np.ascontiguousarray(a[1][:, :k]).tobytes()


def test_phiNearest_of_a_pedigree_names_the_probands(gen, synth_case, synth_ref):
    ped, pro, _, _, _ = synth_case
    got = gen.phiNearest(ped, probandIDs=pro, device=0)
    assert got.k == 10 and PN.same((got.index, got.kinship), tuple(np.ascontiguousarray(a[:, :10]) for a in synth_ref))
    assert np.array_equal(got.pro, pro) and np.array_equal(got.relative, pro[got.index]) and got.relative.dtype == np.int64


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1027])
def test_row_and_tile_edges(gen, synth_case, n):
    ped, pro, _, _, _ = synth_case
    pl = gen.plan(ped, pro[100:100 + n])
    try:
        phi = pl.compute(device=0)
        assert phi.shape == (n, n)
        _check(pl, phi, min(n - 1, 64))                                         # (k = N - 1 where N <= 65: every candidate, in order)
        if n > 2:
            _check(pl, phi, 1)
    finally:
        pl.close()


def test_row_shards_stack_to_the_full_result(synth_case, synth_ref):
    _, _, pl, phi, _ = synth_case
    n = len(phi)
    try:
        parts = []
        for rows in ((0, 1111), (1111, 1111), (1111, 1790), (1790, n)):         # a split off every alignment, one shard empty
            pl.compute_device(device=0, rows=rows)
            parts.append(pl.nearest(64))
        assert [len(p[0]) for p in parts] == [1111, 0, 679, 710] and parts[1][0].shape == parts[1][1].shape == (0, 64)
        assert PN.same(tuple(np.concatenate(x) for x in zip(*parts)), synth_ref)
        pl.compute_device(device=0, rows=(n - 1, n))
        _check(pl, phi[n - 1:], 10, row_begin=n - 1)
    finally:
        pl.compute_device(device=0)                                          # (the module's plan holds the full result again)
    assert PN.same(pl.nearest(64), synth_ref)


# ---- ties and the worst order -----------------------------------------------------------------------------------------------------

def _families(n_unrelated, n_sibs=80):
    """A pedigree of n_unrelated founders without relatives and two sibships of n_sibs first cousins each (two brothers' children).
    Returns (dict for gen.genealogy, unrelated IDs, sibship A, sibship B).  Kinships: 1/4 between full sibs, 1/16 between first
    cousins, 0 with and among the unrelated."""
    ind, fa, mo, sex = [], [], [], []

    def add(i, f, m, s):
        ind.append(i); fa.append(f); mo.append(m); sex.append(s)

    add(1, 0, 0, 1); add(2, 0, 0, 2)                                            # the grandparents
    add(3, 1, 2, 1); add(4, 1, 2, 1)                                            # two brothers
    add(5, 0, 0, 2); add(6, 0, 0, 2)                                            # their wives
    nxt = 7
    sib_a = list(range(nxt, nxt + n_sibs)); nxt += n_sibs
    sib_b = list(range(nxt, nxt + n_sibs)); nxt += n_sibs
    for c in sib_a:
        add(c, 3, 5, 1 + c % 2)
    for c in sib_b:
        add(c, 4, 6, 1 + c % 2)
    unrelated = list(range(nxt, nxt + n_unrelated))
    for u in unrelated:
        add(u, 0, 0, 1 + u % 2)
    return {"ind": ind, "father": fa, "mother": mo, "sex": sex}, unrelated, sib_a, sib_b


def test_unrelated_founders_list_the_first_columns(gen):
    """An all-zero off-diagonal: every candidate ties, row i lists the first k columns, skipping i."""
    ped, unrelated, _, _ = _families(300)
    pl = gen.plan(gen.genealogy(ped), unrelated)
    try:
        phi = pl.compute(device=0)
        assert np.count_nonzero(phi) == 300 and np.all(np.diag(phi) == 0.5)
        for k in (1, 64):
            cols, vals = _check(pl, phi, k)
            assert np.all(vals == 0)
            for i in (0, 1, 63, 64, 65, 299):
                assert cols[i].tolist() == [j for j in range(k + 1) if j != i][:k]
    finally:
        pl.close()


def test_more_than_64_equal_values_at_the_top_and_a_tie_at_the_cut(gen):
    ped, unrelated, sib_a, sib_b = _families(40)
    pro = unrelated[:20] + sib_b + unrelated[20:] + sib_a                        # N = 200
    pl = gen.plan(gen.genealogy(ped), pro)
    try:
        phi = pl.compute(device=0)
        assert sorted(set(phi[199].tolist())) == [0.0, 0.0625, 0.25, 0.5] and np.count_nonzero(phi[199] == 0.25) == 79
        for k in (10, 63, 64):
            cols, vals = _check(pl, phi, k)
            more = pl.nearest(k + 1)[1] if k < 64 else None
            assert np.all(vals[20:100] == 0.25) and np.all(vals[120:] == 0.25)    # 79 equal candidates: the smaller columns win
            assert cols[199].tolist() == list(range(120, 120 + k)) and cols[120].tolist() == list(range(121, 121 + k))
            if more is not None:
                assert np.array_equal(more[:, k - 1], more[:, k])                   # the k-th and the (k + 1)-th candidate tie
        assert PN.same(pl.nearest(64), PN.nearest_literal(phi, 64))
    finally:
        pl.close()


@pytest.fixture(scope="module")
def worst_case(gen):
    """8,460 probands -- three tiles, the last one ragged -- ordered so that a row of sibship A meets better candidates in every
    tile: 4,100 unrelated, its 80 first cousins (sibship B, columns 4,100 .. 4,179: the second tile), 4,200 unrelated, then its
    own sibship (columns 8,380 .. 8,459: the third tile).  (pedigree, proband IDs in that order)."""
    ped, unrelated, sib_a, sib_b = _families(8300)
    return gen.genealogy(ped), np.array(unrelated[:4100] + sib_b + unrelated[4100:] + sib_a, dtype=np.int64)


@pytest.mark.parametrize("order", ["relatives last", "reversed"])
def test_worst_order_with_the_smallest_buffer_and_the_default_one(gen, worst_case, order):
    """Relatives last: the values of a row of sibship A ascend from tile to tile (0, then 1/16, then 1/4).  With the buffer forced
    to 128 keys the first tile overflows it many times over (4,095 zeros, all above tau = 0), the second brings 80 cousins to the
    64 kept (144 > 128) and the third 79 sibs (143 > 128): the buffer is cut in every tile.  The default buffer (1,024 keys) is cut
    in the first tile only.  The answers are the same bytes, and the oracle's."""
    ped, pro = worst_case
    n = len(pro)
    assert n == 8460 and 2 * TILE < n < 3 * TILE
    own, cousins, nobody = slice(n - 80, n), slice(4100, 4180), slice(4000, 4100)       # rows of sibship A, of sibship B, unrelated
    if order == "reversed":
        pro = pro[::-1].copy()
        own, cousins, nobody = slice(0, 80), slice(n - 4180, n - 4100), slice(n - 4100, n - 4000)
    got = {}
    for buf in (128, None, 1000):
        pl = gen.plan(ped, pro, tuning={} if buf is None else {"NEAREST_BUF": buf})
        try:
            phi = pl.compute(device=0)
            assert pl.stats.nearest_buf == {128: 128, None: 1024, 1000: 512}[buf]   # the size used (a power of two in [128, 4096])
            assert np.all(phi[own, own][~np.eye(80, dtype=bool)] == 0.25) and np.all(phi[own, cousins] == 0.0625)
            assert np.count_nonzero(phi[nobody]) == 100
            for k in (64, 10) if buf != 1000 else (64,):
                cols, vals = _check(pl, phi, k, rows=own)
                _check(pl, phi, k, rows=cousins)
                _check(pl, phi, k, rows=nobody)                                      # all zeros: the first columns
                assert np.all(vals[own] == 0.25) and np.all(vals[cousins] == 0.25) and np.all(vals[nobody] == 0)
                got[buf, k] = (cols, vals)
        finally:
            pl.close()
    for k in (64, 10):
        assert PN.same(got[128, k], got[None, k]), k
    assert PN.same(got[1000, 64], got[None, 64])


# ---- genea140 -------------------------------------------------------------------------------------------------------------------

def test_genea140_against_the_committed_oracle_matrix(gen):
    golden = np.load(GOLDEN140)
    ped = gen.genealogy(gen.genea140)
    pl = gen.plan(ped)
    try:
        pl.compute_device(device=0)
        assert PN.same(pl.nearest(10), PN.nearest_numpy(golden, 10))
        assert PN.same(pl.nearest(64), PN.nearest_literal(golden, 64))
    finally:
        pl.close()
    got = gen.phiNearest(ped, device=0)
    assert PN.same((got.index, got.kinship), PN.nearest_numpy(golden, 10)) and np.array_equal(got.relative, gen.pro(ped)[got.index])


# ---- errors -----------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_plan_usable(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(4000, 400, 10, skip_permille=50)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    L, C = gen._capi.lib(), gen._capi
    out = np.full((400, 64), -7, np.int32)
    pc = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    try:
        with pytest.raises(gen.GenphiDeviceError):                        # no resident result yet
            pl.nearest(10)
        assert L.genphi_result_nearest(pl._h, 10, pc, None) == C.GENPHI_ERR_DEVICE
        phi = pl.compute(device=0)
        sums = pl.result_sums()

        def good():
            _check(pl, phi, 10)
            assert pl.result_sums() == sums and np.array_equal(pl.result_to_host(), phi)

        good()
        for k in (0, 400, 65):                                            # k = 0, k = N, k = 65
            with pytest.raises(ValueError):
                pl.nearest(k)
            assert L.genphi_result_nearest(pl._h, k, pc, None) == C.GENPHI_ERR_ARG
            good()
        assert np.all(out == -7)
        pl.compute_device(device=0, storage64=True)                       # a Float64 result
        with pytest.raises(ValueError, match="Float32"):
            pl.nearest(10)
        assert L.genphi_result_nearest(pl._h, 10, pc, None) == C.GENPHI_ERR_ARG
        pl.compute_device(device=0)
        good()
        pl.release_device()
        with pytest.raises(gen.GenphiDeviceError):
            pl.nearest(10)
        assert L.genphi_result_nearest(pl._h, 10, pc, None) == C.GENPHI_ERR_DEVICE
        pl.compute_device(device=0)
        good()
    finally:
        pl.close()
