"""Host side of gen.phiNearest (no GPU): the two selections of tests/phi_nearest_oracle.py against each other, gen.phiNearest on a
host matrix, the known answer of geneaJi, the exported symbol, the test hook, and the argument checks genphi_result_nearest makes
on a plan that has never computed."""
import ctypes
import os
import re

import numpy as np
import pytest

import phi_nearest_oracle as PN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN140 = os.path.join(ROOT, "tests", "golden", "genea140_phi_oracle.npy")

# the reference's pinned kinships of geneaJi's probands 1, 2 and 29 (test/runtests.jl)
PHI_JI = np.array([[0.591796875, 0.37109375, 0.072265625], [0.37109375, 0.591796875, 0.072265625],
                   [0.072265625, 0.072265625, 0.53515625]], dtype=np.float32)


def _random_matrices():
    """50 symmetric non-negative Float32 matrices, N = 2 .. 40, of few distinct values with many zeros: ties everywhere."""
    rng = np.random.default_rng(20261018)
    out = []
    for t in range(50):
        n = 2 + (t * 7) % 39 if t >= 4 else (2, 3, 40, 39)[t]
        a = (rng.integers(0, 5, (n, n)) * rng.integers(0, 2, (n, n))).astype(np.float32) / 16
        out.append(np.maximum(a, a.T))
    assert {len(m) for m in out} >= {2, 3, 39, 40}
    return out


RANDOM = _random_matrices()


def _ks(n):
    return sorted({1, 2, (n - 1) // 2, n - 2, n - 1} & set(range(1, min(n - 1, 64) + 1)))


def test_oracle_on_a_case_computed_by_hand():
    phi = np.array([[.5, .25, .125, 0], [.25, .5, 0, .125], [.125, 0, .5, .125], [0, .125, .125, .5]], dtype=np.float32)
    for f in (PN.nearest_literal, PN.nearest_numpy):
        c, v = f(phi, 2)
        assert c.tolist() == [[1, 2], [0, 3], [0, 3], [1, 2]] and c.dtype == np.int32 and v.dtype == np.float32
        assert v.tolist() == [[.25, .125], [.25, .125], [.125, .125], [.125, .125]]
        c, v = f(phi[2:], 3, row_begin=2)                                    # a shard: rows 2 and 3; never the diagonal
        assert c.tolist() == [[0, 3, 1], [1, 2, 0]] and v.tolist() == [[.125, .125, 0], [.125, .125, 0]]


def test_the_two_oracles_agree_on_random_matrices_with_ties():
    for phi in RANDOM:
        for k in _ks(len(phi)):
            a, b = PN.nearest_literal(phi, k), PN.nearest_numpy(phi, k)
            assert PN.same(a, b), (len(phi), k)
            assert all(i not in a[0][i] for i in range(len(phi))) and a[0].max() < len(phi)


def test_the_two_oracles_agree_on_genea140():
    phi = np.load(GOLDEN140)
    assert phi.shape == (140, 140) and phi.dtype == np.float32
    for k in (1, 10, 64, 139):
        assert PN.same(PN.nearest_literal(phi, k), PN.nearest_numpy(phi, k)), k
    parts = [PN.nearest_numpy(phi[a:b], 10, row_begin=a) for a, b in ((0, 17), (17, 17), (17, 101), (101, 140))]
    assert PN.same(PN.nearest_numpy(phi, 10), tuple(np.concatenate(x) for x in zip(*parts)))
    assert PN.same(PN.nearest_literal(phi[17:101], 10, row_begin=17), parts[2])


def test_phiNearest_of_a_host_matrix_is_the_literal_oracle(gen):
    for phi in RANDOM + [np.load(GOLDEN140)]:
        for k in _ks(len(phi)):
            got = gen.phiNearest(phi, k)
            assert PN.same((got.index, got.kinship), PN.nearest_literal(phi, k)), (len(phi), k)
            assert got.k == k and got.pro is None and got.relative is None and len(got) == len(phi)


def test_geneaJi_known_answer_the_tie_goes_to_the_smaller_column(gen):
    got = gen.phiNearest(PHI_JI, 2, probandIDs=[1, 2, 29])
    assert got.index.tolist() == [[1, 2], [0, 2], [0, 1]]
    assert got.kinship.tolist() == [[0.37109375, 0.072265625], [0.37109375, 0.072265625], [0.072265625, 0.072265625]]
    assert got.relative.tolist() == [[2, 29], [1, 29], [1, 2]] and got.pro.tolist() == [1, 2, 29]
    assert got.index.dtype == np.int32 and got.kinship.dtype == np.float32 and got.relative.dtype == np.int64
    assert "2 nearest relatives of 3 probands" in repr(got)
    for f in (PN.nearest_literal, PN.nearest_numpy):
        assert PN.same(f(PHI_JI, 2), (got.index, got.kinship))


def test_k_is_clipped_and_relative_comes_from_the_ids(gen):
    phi = np.load(GOLDEN140)
    ids = 1000 + 7 * np.arange(140)
    got = gen.phiNearest(PHI_JI, 10)                                        # default-sized k on 3 probands: N - 1
    assert got.k == 2 and got.index.shape == (3, 2)
    assert gen.phiNearest(PHI_JI).k == 2                                    # k = 10 is the default
    got = gen.phiNearest(phi[:65, :65], 1000)
    assert got.k == 64 and PN.same((got.index, got.kinship), PN.nearest_numpy(phi[:65, :65], 64))
    got = gen.phiNearest(phi, 10, probandIDs=ids)
    assert np.array_equal(got.relative, ids[got.index]) and np.array_equal(got.pro, ids) and got.index.shape == (140, 10)


def test_every_value_error(gen):
    phi = np.load(GOLDEN140)
    for k in (0, -3):
        with pytest.raises(ValueError):
            gen.phiNearest(phi, k)
    with pytest.raises(ValueError):
        gen.phiNearest(phi, 65)                                             # 65 <= N - 1 stays 65: above the limit
    with pytest.raises(ValueError):
        gen.phiNearest(phi, 1000)                                           # clipped to 139: above the limit
    with pytest.raises(ValueError):
        gen.phiNearest(phi[:1, :1], 1)                                      # N < 2
    with pytest.raises(ValueError):
        gen.phiNearest(np.zeros((0, 0), np.float32), 1)
    with pytest.raises(ValueError):
        gen.phiNearest(phi[:3], 1)                                          # not square
    with pytest.raises(ValueError):
        gen.phiNearest(phi, 1, probandIDs=[1, 2, 3])
    ped = gen.genealogy(gen.geneaJi)                                        # the same checks come before any device work
    with pytest.raises(KeyError):
        gen.phiNearest(ped, 1, probandIDs=[1, 12345])
    with pytest.raises(ValueError):
        gen.phiNearest(ped, 0)
    with pytest.raises(ValueError):
        gen.phiNearest(ped, 1, probandIDs=[29, 29])                         # one proband after duplicates collapse


def test_symbol_is_exported_declared_and_bound(gen):
    from genlib_jl_amd import _capi
    assert "genphi_result_nearest" in _capi.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), "genphi_result_nearest")
    header = open(os.path.join(ROOT, "include", "genphi.h")).read()
    assert re.search(r"\bgenphi_result_nearest\s*\(", header)
    assert int(re.search(r"#define\s+GENPHI_NEAREST_MAX_K\s+(\d+)", header).group(1)) == _capi.GENPHI_NEAREST_MAX_K == 64
    assert len(_capi.lib().genphi_result_nearest.argtypes) == 4
    assert callable(gen.phiNearest) and isinstance(gen.PhiNearest, type)


def test_the_buffer_hook_is_a_known_setting(gen):
    ped = gen.genealogy(gen.geneaJi)
    for name in ("NEAREST_BUF", "GENPHI_NEAREST_BUF"):
        gen.plan(ped, tuning={name: 128}).close()
    with pytest.raises(ValueError):
        gen.plan(ped, tuning={"NEAREST_BUFFER": 128})
    assert "GENPHI_NEAREST_BUF" in open(os.path.join(ROOT, "README.md")).read()


def test_argument_errors_on_a_plan_that_has_never_computed(gen):
    """What the entry point does without a result, pinned: it checks its arguments first (GENPHI_ERR_ARG), the result last
    (GENPHI_ERR_DEVICE)."""
    ped = gen.genealogy(gen.geneaJi)
    pl = gen.plan(ped)
    L, C = gen._capi.lib(), gen._capi
    cols, vals = np.full((3, 2), -7, np.int32), np.full((3, 2), -7, np.float32)
    pc, pv = cols.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), vals.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    try:
        assert L.genphi_result_nearest(None, 1, pc, pv) == C.GENPHI_ERR_ARG
        assert L.genphi_result_nearest(pl._h, 1, pc, pv) == C.GENPHI_ERR_DEVICE
        assert "no resident result" in C.last_error()
        assert L.genphi_result_nearest(pl._h, 2, pc, None) == C.GENPHI_ERR_DEVICE
        assert L.genphi_result_nearest(pl._h, 2, None, pv) == C.GENPHI_ERR_DEVICE
        assert L.genphi_result_nearest(pl._h, 1, None, None) == C.GENPHI_ERR_ARG          # arguments before the result
        assert "both NULL" in C.last_error()
        for k in (0, -1, 3, 65):
            assert L.genphi_result_nearest(pl._h, k, pc, pv) == C.GENPHI_ERR_ARG, k
            assert "outside [1, 2]" in C.last_error()
        assert np.all(cols == -7) and np.all(vals == -7)
        with pytest.raises(gen.GenphiDeviceError):
            pl.nearest(1)
        for k in (0, 3, 65):
            with pytest.raises(ValueError):
                pl.nearest(k)
        with pytest.raises(ValueError):
            pl.nearest(1, cols=False, values=False)
    finally:
        pl.close()
    pl = gen.plan(ped, [29])                                                # N < 2: nobody has a nearest relative
    try:
        assert L.genphi_result_nearest(pl._h, 1, pc, pv) == C.GENPHI_ERR_ARG
        with pytest.raises(ValueError):
            pl.nearest(1)
    finally:
        pl.close()
