"""Host side of gen.phiOver (no GPU): the two forms of the oracle of tests/phi_over_oracle.py against each other, gen.phiOver on a
host matrix, the exported symbol, and the argument checks genphi_result_over makes on a plan that has never computed."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import phi_over_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN140 = os.path.join(ROOT, "tests", "golden", "genea140_phi_oracle.npy")


def test_oracle_on_a_case_computed_by_hand():
    phi = np.array([[.5, .25, .125, 0], [.25, .5, 0, .125], [.125, 0, .5, .0625], [0, .125, .0625, .5]], dtype=np.float32)
    r, c, v = PO.over(phi, .125)
    assert r.tolist() == [0, 0, 1] and c.tolist() == [1, 2, 3] and v.tolist() == [.25, .125, .125]
    assert r.dtype == np.int32 and c.dtype == np.int32 and v.dtype == np.float32
    r, c, v = PO.over(phi[2:], 0.0, row_begin=2)                            # a shard: rows 2 and 3; never the diagonal
    assert r.tolist() == [2] and c.tolist() == [3] and v.tolist() == [.0625]
    assert len(PO.over(phi, .5)[0]) == 0 and len(PO.over(phi, -math.inf)[0]) == 6 and len(PO.over(phi, math.inf)[0]) == 0


def test_the_two_oracle_forms_agree_on_genea140():
    phi = np.load(GOLDEN140)
    assert phi.shape == (140, 140) and phi.dtype == np.float32
    for t in [0.0, -1.0, math.inf, -math.inf] + [2.0 ** -e for e in range(1, 14)] + [float(phi[0, 1]), float(np.max(np.triu(phi, 1)))]:
        assert PO.same(PO.over(phi, t), PO.over_numpy(phi, t)), t
    for r0, r1 in ((0, 1), (139, 140), (17, 101)):
        assert PO.same(PO.over(phi[r0:r1], 2.0 ** -8, row_begin=r0), PO.over_numpy(phi[r0:r1], 2.0 ** -8, row_begin=r0))
    full = PO.over_numpy(phi, 2.0 ** -8)
    parts = [PO.over_numpy(phi[a:b], 2.0 ** -8, row_begin=a) for a, b in ((0, 17), (17, 101), (101, 140))]
    assert 0 < len(full[0]) < 140 * 139 // 2 and PO.same(full, tuple(np.concatenate(x) for x in zip(*parts)))


@pytest.mark.parametrize("n", [1, 2, 5, 33])
def test_the_two_oracle_forms_agree_on_random_matrices_with_ties(n):
    rng = np.random.default_rng(n)
    a = rng.integers(0, 6, (n, n)).astype(np.float32) / 8                   # few distinct values: ties at every threshold
    phi = np.maximum(a, a.T)
    for t in (0.0, .125, .25, .3, .625, .75, -0.0):
        got = PO.over(phi, t)
        assert PO.same(got, PO.over_numpy(phi, t))
        assert len(got[0]) == sum(1 for i in range(n) for j in range(i + 1, n) if phi[i, j] >= t)


def test_phiOver_of_a_host_matrix_is_the_oracle(gen):
    phi = np.load(GOLDEN140)
    ids = 1000 + 7 * np.arange(140)
    for t in (2.0 ** -6, 0.0, 1.0):
        ref = PO.over_numpy(phi, t)
        got = gen.phiOver(phi, t)
        assert PO.same((got.row, got.col, got.kinship), ref) and got.pro1 is None and got.pro2 is None and len(got) == len(ref[0])
        got = gen.phiOver(phi, t, probandIDs=ids)
        assert PO.same((got.row, got.col, got.kinship), ref)
        assert np.array_equal(got.pro1, ids[ref[0]]) and np.array_equal(got.pro2, ids[ref[1]]) and got.pro1.dtype == np.int64
    assert "pairs" in repr(gen.phiOver(phi, 2.0 ** -6, probandIDs=ids)) and len(gen.phiOver(phi, 1.0)) == 0
    with pytest.raises(ValueError):
        gen.phiOver(phi, math.nan)
    with pytest.raises(ValueError):
        gen.phiOver(phi[:3], 0.1)                                           # not square
    with pytest.raises(ValueError):
        gen.phiOver(phi, 0.1, probandIDs=ids[:5])


def test_unknown_id_and_nan_raise_before_any_device_work(gen):
    ped = gen.genealogy(gen.geneaJi)
    with pytest.raises(KeyError):
        gen.phiOver(ped, 0.1, probandIDs=[1, 12345])
    with pytest.raises(ValueError):
        gen.phiOver(ped, math.nan)


def test_symbol_is_exported_declared_and_bound(gen):
    from genlib_jl_amd import _capi
    assert "genphi_result_over" in _capi.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), "genphi_result_over")
    header = open(os.path.join(ROOT, "include", "genphi.h")).read()
    assert re.search(r"\bgenphi_result_over\s*\(", header)
    assert len(_capi.lib().genphi_result_over.argtypes) == 7


def test_argument_errors_on_a_plan_that_has_never_computed(gen):
    ped = gen.genealogy(gen.geneaJi)
    pl = gen.plan(ped)
    L, C = gen._capi.lib(), gen._capi
    n = ctypes.c_int64(-7)
    try:
        assert L.genphi_result_over(pl._h, 0.1, 0, None, None, None, ctypes.byref(n)) == C.GENPHI_ERR_DEVICE and n.value == 0
        assert "no resident result" in C.last_error()
        assert L.genphi_result_over(pl._h, math.nan, 0, None, None, None, ctypes.byref(n)) == C.GENPHI_ERR_ARG
        assert "NaN" in C.last_error()
        assert L.genphi_result_over(pl._h, 0.1, -1, None, None, None, None) == C.GENPHI_ERR_ARG
        assert L.genphi_result_over(None, 0.1, 0, None, None, None, None) == C.GENPHI_ERR_ARG
        with pytest.raises(gen.GenphiDeviceError):
            pl.phi_over(0.1)
        with pytest.raises(gen.GenphiDeviceError):
            pl.count_over(0.1)
        with pytest.raises(ValueError):
            pl.phi_over(math.nan)
        with pytest.raises(ValueError):
            pl.count_over(math.nan)
    finally:
        pl.close()
    pl = gen.plan(ped, [29])                                                # N < 2: no pair exists, with or without a result
    try:
        assert L.genphi_result_over(pl._h, -math.inf, 0, None, None, None, ctypes.byref(n)) == 0 and n.value == 0
        assert pl.count_over(0.0) == 0 and all(len(a) == 0 for a in pl.phi_over(0.0))
    finally:
        pl.close()
