"""gen.occ and gen.rec on the GPU (csrc/occ.hip) against the oracles of tests/occ_oracle.py and the reference's pins.  Every
comparison is exact (np.array_equal on int64).  Every occ case runs with both row widths where 32-bit rows are allowed (sweeps of
at most 31 steps), as a full result and as device-reduced totals, and the totals must equal the row sums of the full result."""
import ctypes

import numpy as np
import pytest

from occ_oracle import occ_exact, occ_literal, rec_exact, rec_literal
from test_gc_gpu import _mixed_lists, _one_parent_synth
from test_occ_reference import (G140, JI_OCC, JI_REC, JI_TOTAL, QUIRK_ANC, QUIRK_OCC, QUIRK_PRO, QUIRK_REC, QUIRK_REC_PRO,
                                QUIRK_TOTAL, doubling_chain, quirk_pedigree)

pytestmark = pytest.mark.gpu


def _ped(gen, ind, fa, mo, sex=None, sort=True):
    sex = np.ones(len(ind), dtype=np.int64) if sex is None else sex
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}, sort=sort)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.int64 and a.shape == b.shape, (a.dtype, a.shape, b.shape)
    bad = np.argwhere(a != b)
    assert len(bad) == 0, f"{len(bad)} entries differ, first at {tuple(bad[0])}: {a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}"


def _occ_all_ways(gen, ped, pro, anc, expect_bits=None):
    """occ of (pro, anc) as the full result and as totals, with the default row width and with 64-bit rows forced: all equal.
    Returns the (n_anc, n_pro) result and the (n_anc, 1) totals."""
    pro, anc = np.asarray(pro, dtype=np.int64), np.asarray(anc, dtype=np.int64)
    results, totals, widths = [], [], []
    for rows64 in (False, True):
        h = gen.OccPlan(ped.ind, ped.father, ped.mother, pro, anc, rows64=rows64)
        t = gen.OccPlan(ped.ind, ped.father, ped.mother, pro, anc, total_only=True, rows64=rows64)
        try:
            h.compute()
            t.compute()
            widths.append(h.stats()["row_bits"])
            assert t.stats()["row_bits"] == widths[-1]
            results.append(h.result_to_host())
            totals += [t.totals(), h.totals()]               # reduced by the last step / column sums of the resident result
        finally:
            h.close()
            t.close()
    assert widths[1] == 64 and widths[0] in (32, 64)
    if expect_bits is not None:
        assert widths[0] == expect_bits
    _same(results[0], results[1])
    for t in totals:
        _same(t, results[0].sum(axis=0, dtype=np.int64))
    return results[0].T, totals[0].reshape(-1, 1)


def _check(gen, ped, pro, anc, exact=False, rec_pro=None):
    occ_ref, rec_ref = (occ_exact, rec_exact) if exact else (occ_literal, rec_literal)
    occ, total = _occ_all_ways(gen, ped, pro, anc)
    _same(occ, occ_ref(ped.ind, ped.father, ped.mother, pro, anc))
    _same(gen.occ(ped, pro=pro, ancestors=anc), occ)
    _same(gen.occ(ped, pro=pro, ancestors=anc, typeOcc="TOTAL"), total)
    rec_pro = pro if rec_pro is None else rec_pro
    _same(gen.rec(ped, rec_pro, anc), rec_ref(ped.ind, ped.father, ped.mother, rec_pro, anc))
    return occ


@pytest.fixture(scope="module")
def genea140(gen):
    ped = gen.genealogy(gen.genea140)
    return ped, gen.pro(ped), gen.founder(ped)


@pytest.fixture(scope="module")
def genea140_literal(genea140):
    ped, pro, anc = genea140
    occ = occ_literal(ped.ind, ped.father, ped.mother, pro, anc)
    rec = rec_literal(ped.ind, ped.father, ped.mother, pro, anc)
    assert int(occ.sum()) == G140["occ_sum"] and int(rec.sum()) == G140["rec_sum"]      # the oracle is a yardstick only if it holds the pins
    return occ, rec


@pytest.fixture(scope="module")
def synth_one_parent(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, _ = _one_parent_synth(synth)
    return _ped(gen, ind, fa, mo, sex)


def test_geneaJi_default_arguments(gen):
    ped = gen.genealogy(gen.geneaJi)
    _same(gen.occ(ped), JI_OCC)                                     # test/runtests.jl:63
    _same(gen.occ(ped, typeOcc="TOTAL"), JI_TOTAL)                  # :65
    _same(gen.rec(ped), JI_REC)                                     # :66
    _same(_check(gen, ped, gen.pro(ped), gen.founder(ped)), JI_OCC)


def test_genea140_default_arguments(gen, genea140, genea140_literal):
    ped, pro, anc = genea140
    occ, total = _occ_all_ways(gen, ped, pro, anc, expect_bits=32)
    _same(occ, genea140_literal[0])
    _same(gen.occ(ped), genea140_literal[0])
    assert int(occ.sum()) == G140["occ_sum"] and int(occ.max()) == G140["occ_max"]
    _same(gen.occ(ped, typeOcc="TOTAL"), total)
    assert total.shape == (7399, 1) and int(total.max()) == G140["total_max"]
    rec = gen.rec(ped)
    _same(rec, genea140_literal[1])
    assert int(rec.sum()) == G140["rec_sum"] and int(rec.max()) == G140["rec_max"]


@pytest.mark.parametrize("panel", [1, 3, 64, 65])
def test_genea140_column_panels(gen, genea140, genea140_literal, monkeypatch, panel):
    """7,399 founders in panels of 1, 3 (a ragged last panel of 1), 64 (ragged: 39) and 65 columns (ragged: 54; every panel's bit
    rows end inside their second word, and panel boundaries fall inside the words of a 64-column grid), all panels in one
    launch through grid dimension y."""
    monkeypatch.setenv("GENPHI_OCC_PANEL", str(panel))
    ped, pro, anc = genea140
    occ, _ = _occ_all_ways(gen, ped, pro, anc)
    _same(occ, genea140_literal[0])
    h = gen.RecPlan(ped.ind, ped.father, ped.mother, pro, anc)
    try:
        h.compute()
        st = h.stats()
        assert st["panel_cols"] == panel
        assert st["launches"] < 2 * (7399 // panel + 1)            # fewer launches than panels x lists: several panels per launch
        _same(h.result(), genea140_literal[1])
    finally:
        h.close()


@pytest.mark.parametrize("group", [1, 7])
def test_genea140_panels_per_launch(gen, genea140, genea140_literal, monkeypatch, group):
    """Panels of 100 columns (rec: two words, the second ragged), one and seven per launch (the last launch holds four)."""
    monkeypatch.setenv("GENPHI_OCC_PANEL", "100")
    monkeypatch.setenv("GENPHI_OCC_PANELS_PER_LAUNCH", str(group))
    ped, pro, anc = genea140
    occ, _ = _occ_all_ways(gen, ped, pro, anc)
    _same(occ, genea140_literal[0])
    _same(gen.rec(ped), genea140_literal[1])


def test_row_width_hook(gen, genea140, genea140_literal, monkeypatch):
    monkeypatch.setenv("GENPHI_OCC_ROWS", "64")
    ped, pro, anc = genea140
    h = gen.OccPlan(ped.ind, ped.father, ped.mother, pro, anc)
    try:
        h.compute()
        assert h.stats()["row_bits"] == 64
        _same(h.result_to_host().T, genea140_literal[0])
    finally:
        h.close()


def test_hand_built_quirks(gen):
    """Non-founder ancestors, ancestors that are probands, probands with children (the father of another proband; one three cuts
    above the last), a repeated proband, a duplicated ancestor (occ: later row zero; rec: equal), a proband ID unknown to rec."""
    ped = quirk_pedigree(gen)
    occ, total = _occ_all_ways(gen, ped, QUIRK_PRO, QUIRK_ANC, expect_bits=32)
    _same(occ, QUIRK_OCC)
    _same(total, QUIRK_TOTAL)
    _same(gen.occ(ped, pro=QUIRK_PRO, ancestors=QUIRK_ANC), QUIRK_OCC)
    _same(gen.occ(ped, pro=QUIRK_PRO, ancestors=QUIRK_ANC, typeOcc="TOTAL"), QUIRK_TOTAL)
    _same(gen.rec(ped, QUIRK_REC_PRO, QUIRK_ANC), QUIRK_REC)
    _same(gen.rec(ped, QUIRK_PRO, QUIRK_ANC), QUIRK_REC)


def test_errors_and_empty_lists(gen, genea140):
    ped, pro, anc = genea140
    with pytest.raises(KeyError):
        gen.occ(ped, pro=[int(pro[0]), 10 ** 9])
    with pytest.raises(KeyError):
        gen.occ(ped, ancestors=[int(anc[0]), 10 ** 9])
    with pytest.raises(KeyError):
        gen.rec(ped, pro, [10 ** 9])
    with pytest.raises(ValueError):
        gen.occ(ped, typeOcc="total")
    assert gen.occ(ped, pro=[], ancestors=anc[:5]).shape == (5, 0)
    assert gen.occ(ped, pro=pro[:4], ancestors=[]).shape == (0, 4)
    _same(gen.occ(ped, pro=[], ancestors=anc[:5], typeOcc="TOTAL"), np.zeros((5, 1), dtype=np.int64))
    assert gen.occ(ped, pro=pro[:4], ancestors=[], typeOcc="TOTAL").shape == (0, 1)
    _same(gen.rec(ped, [], anc[:5]), np.zeros(5, dtype=np.int64))
    _same(gen.rec(ped, [10 ** 9], anc[:5]), np.zeros(5, dtype=np.int64))
    assert gen.rec(ped, pro[:4], []).shape == (0,)


@pytest.mark.parametrize("n_anc", [13, 63, 130])
def test_genea140_mixed_lists(gen, genea140, n_anc):
    """Unsorted, repeated, non-leaf and founder probands; non-founder, duplicated and proband ancestors; 130 columns: three words."""
    ped, _, _ = genea140
    pro, anc = _mixed_lists(ped, gen, np.random.default_rng(n_anc), n_anc)
    _check(gen, ped, pro, anc, rec_pro=np.concatenate([pro, [10 ** 9]]))


def test_one_parent_synthetic(gen, synth_one_parent):
    ped = synth_one_parent
    pro, anc = _mixed_lists(ped, gen, np.random.default_rng(5), 21)
    _check(gen, ped, pro, anc, exact=True)
    _check(gen, ped, gen.pro(ped), gen.founder(ped)[:300], exact=True)


def test_unsorted_ranks(gen):
    """sort=false: ranks follow a parents-first file order, not the depth."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, _ = _one_parent_synth(synth)
    ind, fa, mo, sex = synth.parents_first_shuffle(ind, fa, mo, sex, seed=3)
    ped = _ped(gen, ind, fa, mo, sex, sort=False)
    pro, anc = _mixed_lists(ped, gen, np.random.default_rng(9), 17)
    _check(gen, ped, pro, anc, exact=True)


def test_probands_all_founders(gen, synth_one_parent):
    """Zero level steps: only founders among the probands."""
    ped = synth_one_parent
    f = gen.founder(ped)
    _check(gen, ped, list(f[:5]) + [f[0]], list(f[:4]) + [f[1], f[7]])


def test_wrap_around(gen):
    """A founder's count doubles per generation: 2^62, 2^63 (Int64: -2^63), 2^64 and 2^70 (Int64: 0) paths.  rec still counts
    every such proband: it is not occ > 0, and nothing saturates or passes through floating point."""
    ind, fa, mo = doubling_chain(72)
    ped = _ped(gen, ind, fa, mo)
    pro = [2 * 64, 2 * 65, 2 * 66, 2 * 72]
    anc = [1, 2, 5]
    ref = occ_exact(ped.ind, ped.father, ped.mother, pro, anc)
    assert ref[0].tolist() == [2 ** 62, -2 ** 63, 0, 0] and ref[2].tolist() == [2 ** 60, 2 ** 61, 2 ** 62, 0]      # 5: two generations later
    occ, total = _occ_all_ways(gen, ped, pro, anc, expect_bits=64)
    _same(occ, ref)
    _same(total, occ_exact(ped.ind, ped.father, ped.mother, pro, anc, typeOcc="TOTAL"))
    _same(gen.rec(ped, pro, anc), np.array([4, 4, 4], dtype=np.int64))
    _same(gen.rec(ped, pro, anc), rec_exact(ped.ind, ped.father, ped.mother, pro, anc))


@pytest.mark.parametrize("generations,bits", [(32, 32), (33, 64), (41, 64)])
def test_row_width_follows_the_depth(gen, generations, bits):
    """31 steps: 32-bit rows (the largest count is 2^30); 32 and 40 steps select 64-bit rows on their own (2^39 does not fit)."""
    ind, fa, mo = doubling_chain(generations)
    ped = _ped(gen, ind, fa, mo)
    pro = [2 * generations, 2 * generations - 1, 2 * generations - 2]
    anc = [1, 2, 3]
    occ, _ = _occ_all_ways(gen, ped, pro, anc, expect_bits=bits)
    _same(occ, occ_exact(ped.ind, ped.father, ped.mother, pro, anc))
    assert int(occ[0, 0]) == 2 ** (generations - 2)


def test_cfg3_all_founders(gen):
    """cfg3: 1e4 probands x 6,633 founders.  64 sampled proband rows against the exact counts, the device-reduced totals against
    the column sums of the resident result (taken on the device and on the host), rec against the exact ancestor sets in full."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(100_000, 10_000, 20)
    ped = _ped(gen, ind, fa, mo, sex)
    anc = gen.founder(ped)
    assert len(anc) == 6633
    sample = np.random.default_rng(3).choice(len(pro), 64, replace=False)
    ref = occ_exact(ped.ind, ped.father, ped.mother, pro, anc, sample=sample)
    h = gen.OccPlan(ped.ind, ped.father, ped.mother, pro, anc)
    t = gen.OccPlan(ped.ind, ped.father, ped.mother, pro, anc, total_only=True)
    try:
        h.compute()
        t.compute()
        out = h.result_to_host()
        assert out.shape == (10_000, 6633)
        _same(out[sample].T, ref)
        _same(t.totals(), h.totals())
        _same(t.totals(), out.sum(axis=0, dtype=np.int64))
    finally:
        h.close()
        t.close()
    _same(gen.rec(ped, pro, anc), rec_exact(ped.ind, ped.father, ped.mother, pro, anc))


def test_c_abi_from_plain_ctypes(gen, genea140, genea140_literal):
    """create, compute, result_to_host, destroy through ctypes alone; compute twice gives the same bits; destroy without compute."""
    from genlib_jl_amd import _capi
    ped, pro, anc = genea140
    L = ctypes.CDLL(_capi.LIB_PATH)
    P64 = ctypes.POINTER(ctypes.c_int64)
    arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (ped.ind, ped.father, ped.mother, pro, anc)]
    ptr = [a.ctypes.data_as(P64) for a in arrs]
    n = [ctypes.c_int64(len(a)) for a in arrs]
    L.genphi_occ_destroy.restype = None
    L.genphi_occ_destroy.argtypes = [ctypes.c_void_p]
    L.genphi_rec_destroy.restype = None
    L.genphi_rec_destroy.argtypes = [ctypes.c_void_p]
    h = ctypes.c_void_p()
    assert L.genphi_occ_create(n[0], ptr[0], ptr[1], ptr[2], n[3], ptr[3], n[4], ptr[4], ctypes.c_int32(0), ctypes.byref(h)) == 0
    L.genphi_occ_destroy(h)                                          # never computed
    h = ctypes.c_void_p()
    assert L.genphi_occ_create(n[0], ptr[0], ptr[1], ptr[2], n[3], ptr[3], n[4], ptr[4], ctypes.c_int32(0), ctypes.byref(h)) == 0
    outs = []
    for _ in range(2):
        assert L.genphi_occ_compute(h, ctypes.c_int32(-1)) == 0
        out = np.full((len(pro), len(anc)), -1, dtype=np.int64)
        assert L.genphi_occ_result_to_host(h, out.ctypes.data_as(P64)) == 0
        outs.append(out)
    L.genphi_occ_destroy(h)
    _same(outs[0], outs[1])
    _same(outs[0].T, genea140_literal[0])
    r = ctypes.c_void_p()
    assert L.genphi_rec_create(n[0], ptr[0], ptr[1], ptr[2], n[3], ptr[3], n[4], ptr[4], ctypes.byref(r)) == 0
    L.genphi_rec_destroy(r)
    r = ctypes.c_void_p()
    assert L.genphi_rec_create(n[0], ptr[0], ptr[1], ptr[2], n[3], ptr[3], n[4], ptr[4], ctypes.byref(r)) == 0
    recs = []
    for _ in range(2):
        assert L.genphi_rec_compute(r, ctypes.c_int32(-1)) == 0
        out = np.full(len(anc), -1, dtype=np.int64)
        assert L.genphi_rec_result(r, out.ctypes.data_as(P64)) == 0
        recs.append(out)
    L.genphi_rec_destroy(r)
    _same(recs[0], recs[1])
    _same(recs[0], genea140_literal[1])
