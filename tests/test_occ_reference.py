"""gen.occ (src/describe.jl:184-238) and gen.rec (src/describe.jl:133-145) on the CPU: the two oracles of tests/occ_oracle.py
against each other, against the reference's pins and against hand-written matrices of the reference's quirks; the host-only parts
of the library's gen.occ / gen.rec (argument errors, planning without a GPU, the row width chosen at plan time, exports)."""
import ctypes
import os
import re

import numpy as np
import pytest

from occ_oracle import occ_exact, occ_literal, rec_exact, rec_literal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# test/runtests.jl:63,65,66: geneaJi with default arguments (pro = [1, 2, 29], ancestors = [17, 19, 20, 23, 25, 26])
JI_OCC = np.array([[6, 6, 2], [8, 8, 2], [1, 1, 2], [0, 0, 1], [8, 8, 3], [8, 8, 3]], dtype=np.int64)
JI_TOTAL = np.array([[14], [18], [4], [1], [19], [19]], dtype=np.int64)
JI_REC = np.array([3, 3, 3, 1, 3, 3], dtype=np.int64)
# genea140 with default arguments (140 probands, 7,399 founders): sum and maximum of occ, maximum of TOTAL, sum and maximum of rec
G140 = {"occ_sum": 287_849, "occ_max": 176, "total_max": 2_539, "rec_sum": 90_814, "rec_max": 121}


def _ped(gen, ind, fa, mo, sort=True):
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=sort)


def quirk_pedigree(gen):
    """1, 2, 5, 10, 11 founders; 3 = (1, 2); 4 = (1, -) one parent; 6 = (3, 5); 7 = (3, 4); 8 = (6, 7); 9 = (4, -); 12 = (8, 9) the
    only leaf with parents; 10 and 11 founders without children."""
    ind = np.arange(1, 13)
    fa = np.array([0, 0, 1, 1, 0, 3, 3, 6, 4, 0, 0, 8])
    mo = np.array([0, 0, 2, 0, 0, 5, 4, 7, 0, 0, 0, 9])
    return _ped(gen, ind, fa, mo)


# pro: a leaf, its father (a proband that is a parent of another proband), 3 (three cuts above the last), the leaf again, a
#      founder without children that is also an ancestor, a founder with children that is also an ancestor
# ancestors: 1 twice (only the first row carries values), 3 with parents (1 is requested too: paths run through 3), 8 a proband,
#      10 a proband, 5, 11 unrelated, 4 with one parent
QUIRK_PRO = [12, 8, 3, 12, 10, 1]
QUIRK_ANC = [1, 1, 3, 8, 10, 5, 11, 4]
QUIRK_OCC = np.array([
    [4, 3, 1, 4, 0, 1],     # 1: 8 has 1-3-6-8, 1-3-7-8, 1-4-7-8; 12 = (8, 9) adds 1-4-9-12; 3 has 1-3; 1 itself
    [0, 0, 0, 0, 0, 0],     # 1 again: its counter was reset after being read
    [2, 2, 1, 2, 0, 0],     # 3: through 6 and 7; itself
    [1, 1, 0, 1, 0, 0],     # 8: 12's father; itself
    [0, 0, 0, 0, 1, 0],     # 10: itself only
    [1, 1, 0, 1, 0, 0],     # 5: 5-6-8
    [0, 0, 0, 0, 0, 0],     # 11: unrelated
    [2, 1, 0, 2, 0, 0],     # 4: 4-7-8, 4-9-12
], dtype=np.int64)
QUIRK_TOTAL = np.array([[13], [0], [7], [3], [1], [3], [0], [5]], dtype=np.int64)       # 12 is listed twice and counts twice
# rec: distinct probands 12, 8, 3, 10, 1 (99 is not in the pedigree); strict descendants; the duplicated ancestor gives equal entries
QUIRK_REC_PRO = QUIRK_PRO + [99]
QUIRK_REC = np.array([3, 3, 2, 1, 0, 2, 0, 2], dtype=np.int64)


def doubling_chain(generations):
    """Generation g = two full siblings (IDs 2g - 1, 2g) whose parents are the two siblings of generation g - 1: the number of
    ascending paths from a member of generation g to a founder (generation 1) is 2^(g - 2)."""
    n = 2 * generations
    ind = np.arange(1, n + 1)
    fa, mo = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for g in range(2, generations + 1):
        fa[2 * g - 2] = fa[2 * g - 1] = 2 * g - 3
        mo[2 * g - 2] = mo[2 * g - 1] = 2 * g - 2
    return ind, fa, mo


def test_oracles_reproduce_the_geneaJi_pins(gen):
    ped = gen.genealogy(gen.geneaJi)
    args = (ped.ind, ped.father, ped.mother, gen.pro(ped), gen.founder(ped))
    assert list(args[3]) == [1, 2, 29] and list(args[4]) == [17, 19, 20, 23, 25, 26]
    for occ in (occ_literal, occ_exact):
        assert np.array_equal(occ(*args), JI_OCC)
        assert np.array_equal(occ(*args, typeOcc="TOTAL"), JI_TOTAL)
    for rec in (rec_literal, rec_exact):
        assert np.array_equal(rec(*args), JI_REC)


def test_oracles_reproduce_the_genea140_pins(gen):
    ped = gen.genealogy(gen.genea140)
    args = (ped.ind, ped.father, ped.mother, gen.pro(ped), gen.founder(ped))
    lit = occ_literal(*args)
    assert lit.shape == (7399, 140) and lit.dtype == np.int64
    assert int(lit.sum()) == G140["occ_sum"] and int(lit.max()) == G140["occ_max"]
    assert int(occ_literal(*args, typeOcc="TOTAL").max()) == G140["total_max"]
    assert np.array_equal(lit, occ_exact(*args))
    rec = rec_literal(*args)
    assert int(rec.sum()) == G140["rec_sum"] and int(rec.max()) == G140["rec_max"]
    assert np.array_equal(rec, rec_exact(*args))


def test_quirks_in_both_oracles(gen):
    ped = quirk_pedigree(gen)
    args = (ped.ind, ped.father, ped.mother)
    for occ in (occ_literal, occ_exact):
        assert np.array_equal(occ(*args, QUIRK_PRO, QUIRK_ANC), QUIRK_OCC)
        assert np.array_equal(occ(*args, QUIRK_PRO, QUIRK_ANC, typeOcc="TOTAL"), QUIRK_TOTAL)
        assert occ(*args, QUIRK_PRO, QUIRK_ANC, typeOcc="SUM") is None
    for rec in (rec_literal, rec_exact):
        assert np.array_equal(rec(*args, QUIRK_REC_PRO, QUIRK_ANC), QUIRK_REC)


def test_quirk_unknown_and_empty_in_oracles(gen):
    ped = quirk_pedigree(gen)
    args = (ped.ind, ped.father, ped.mother)
    for occ in (occ_literal, occ_exact):
        with pytest.raises(KeyError):
            occ(*args, [8, 99], [1])
        with pytest.raises(KeyError):
            occ(*args, [8], [99])
        assert occ(*args, [], [1, 2]).shape == (2, 0)
        assert occ(*args, [8, 9], []).shape == (0, 2)
        assert np.array_equal(occ(*args, [], [1, 2], typeOcc="TOTAL"), np.zeros((2, 1), dtype=np.int64))
    for rec in (rec_literal, rec_exact):
        with pytest.raises(KeyError):
            rec(*args, [8], [99])
        assert np.array_equal(rec(*args, [], [1, 2]), [0, 0])
        assert rec(*args, [8], []).shape == (0,)


def test_doubling_chain_wraps_in_the_exact_oracle():
    """2^62, 2^63, 2^64 and 2^70 paths: Int64 reads 2^62, -2^63, 0 and 0; every such proband still descends from the founder."""
    ind, fa, mo = doubling_chain(72)
    pro = [2 * 64, 2 * 65, 2 * 66, 2 * 72]
    big = occ_exact(ind, fa, mo, pro, [1, 2], exact_ints=True)
    assert [int(v) for v in big[0]] == [2 ** 62, 2 ** 63, 2 ** 64, 2 ** 70]
    assert np.array_equal(occ_exact(ind, fa, mo, pro, [1, 2]), np.array([[2 ** 62, -2 ** 63, 0, 0]] * 2, dtype=np.int64))
    assert np.array_equal(rec_exact(ind, fa, mo, pro, [1, 2]), [4, 4])
    assert np.array_equal(rec_literal(ind, fa, mo, pro, [1, 2]), [4, 4])


def test_unknown_ids_and_bad_type_raise_without_gpu(gen):
    ped = quirk_pedigree(gen)
    with pytest.raises(KeyError):
        gen.occ(ped, pro=[8, 99])
    with pytest.raises(KeyError):
        gen.occ(ped, pro=[8], ancestors=[1, 99])
    with pytest.raises(KeyError):
        gen.rec(ped, [8], [1, 99])
    with pytest.raises(KeyError):
        gen.OccPlan(ped.ind, ped.father, ped.mother, [8], [0])
    with pytest.raises(ValueError):
        gen.occ(ped, typeOcc="SUM")
    gen.RecPlan(ped.ind, ped.father, ped.mother, [8, 99], [1]).close()        # an unknown proband is ignored


def test_plans_are_host_only_and_choose_the_row_width(gen):
    """create plans on the host: the handles report their slot rows and row width before any GPU is touched.  32-bit rows while
    the counts provably fit (at most 31 steps), 64-bit rows beyond, or when asked for."""
    ped = gen.genealogy(gen.genea140)
    args = (ped.ind, ped.father, ped.mother, gen.pro(ped), gen.founder(ped))
    for make, bits in ((lambda: gen.OccPlan(*args), 32), (lambda: gen.OccPlan(*args, rows64=True), 64),
                       (lambda: gen.OccPlan(*args, total_only=True), 32), (lambda: gen.RecPlan(*args), 64)):
        h = make()
        try:
            st = h.stats()
            assert st["peak_slots"] > 0 and st["sweep_ms"] == 0.0 and st["row_bits"] == bits
        finally:
            h.close()
    for generations, bits in ((32, 32), (33, 64), (41, 64)):          # 31, 32 and 40 steps
        ind, fa, mo = doubling_chain(generations)
        h = gen.OccPlan(ind, fa, mo, [2 * generations], [1])
        try:
            assert h.stats()["row_bits"] == bits
        finally:
            h.close()


def test_symbols_are_exported_and_called_by_the_julia_shim(gen):
    from genlib_jl_amd import _capi
    src = open(os.path.join(ROOT, "genlib.jl_amd", "julia", "GenLibAMD.jl")).read()
    called = set(re.findall(r"\(:(genphi_(?:occ|rec)_[a-z_]+), libgenphi\)", src))
    assert called == {"genphi_occ_create", "genphi_occ_compute", "genphi_occ_result_to_host", "genphi_occ_totals", "genphi_occ_destroy",
                      "genphi_rec_create", "genphi_rec_compute", "genphi_rec_result", "genphi_rec_destroy"}
    L = ctypes.CDLL(_capi.LIB_PATH)
    for name in called | {"genphi_occ_result_device", "genphi_occ_stats", "genphi_rec_stats"}:
        assert hasattr(L, name), name
