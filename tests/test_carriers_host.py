"""gen.simuCarriers without a GPU: the reference of tests/carriers_oracle.py on hand-made labels and its invariants on a real
pedigree, the host plan of gen.CarriersPlan against gen.IdentityPlan's on cases + controls, every argument error and limit of the
definition (include/genphi.h, genphi_carry_*), the shares of gen.SimuCarriers from hand-made integer tables, and csrc/carry.h as a
stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (tests/carry_check.cpp)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from carriers_oracle import CarryVector, check_invariants, counts, fill, tables
from random_pedigree import random_pedigree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SUMMARY = re.compile(r"^carry check: (\d+) chunk cases, (\d+) chunks walked, (\d+) plans, (\d+) overlaps refused, (\d+) lists with repeats; (\d+) violations$", re.M)

IND = np.arange(1, 10, dtype=np.int64)
FA = np.array([0, 0, 1, 1, 3, 3, 0, 5, 0], dtype=np.int64)
MO = np.array([0, 0, 2, 2, 4, 3, 4, 7, 0], dtype=np.int64)


def _ped(gen, ind, fa, mo):
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)


def _founders(n):
    """n unrelated founders."""
    return np.arange(1, n + 1, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)


def test_the_oracle_on_hand_made_labels():
    """Three cases and one control, five labels, four simulations.
    s = 0: the cases carry (0, 1), (2, 1), (0, 0); the control (4, 4).     s = 1: (0, 0), (0, 1), (4, 3); the control (1, 2).
    s = 2: everyone (1, 1).                                                 s = 3: (3, 4), (3, 3), (3, 3); the control (0, 0)."""
    cases = np.array([[[0, 0, 1, 3], [1, 0, 1, 4]],
                      [[2, 0, 1, 3], [1, 1, 1, 3]],
                      [[0, 4, 1, 3], [0, 3, 1, 3]]], dtype=np.int32)
    control = np.array([[[4, 1, 1, 0], [4, 2, 1, 0]]], dtype=np.int32)
    c1, c2 = counts(cases, 5)
    assert c1.T.tolist() == [[2, 2, 1, 0, 0], [2, 1, 0, 1, 1], [0, 3, 0, 0, 0], [0, 0, 0, 3, 1]]
    assert c2.T.tolist() == [[1, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0, 3, 0, 0, 0], [0, 0, 0, 2, 0]]
    carriers, homozygotes, excluded = tables(cases, control[:0], 5)
    assert excluded.tolist() == [0] * 5
    assert carriers.tolist() == [[0, 0, 2, 0], [0, 1, 1, 1], [0, 1, 0, 0], [0, 1, 0, 1], [0, 2, 0, 0]]
    assert homozygotes.tolist() == [[0, 2, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]]
    assert check_invariants(carriers, homozygotes, excluded, np.array([[10, 0], [10, 1], [20, 1], [30, 0], [30, 1]]), 4, [1, 2, 3]) == 0
    assert fill(carriers, excluded, 4)[:, 0].tolist() == [2, 1, 3, 2, 2]
    carriers, homozygotes, excluded = tables(cases, control, 5)
    assert excluded.tolist() == [1, 2, 1, 0, 1]                           # label 0 at s = 3; 1 at s = 1, 2; 2 at s = 1; 4 at s = 0
    assert carriers.tolist() == [[0, 0, 2, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 1, 0, 1], [0, 2, 0, 0]]
    assert homozygotes.tolist() == [[0, 2, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]]
    lumped, lumped_hom, _ = tables(cases, control, 5, max_count=1)
    assert lumped.tolist() == [[0, 2], [0, 1], [0, 1], [0, 2], [0, 2]] and lumped_hom.tolist() == [[0, 2], [0, 0], [0, 0], [0, 1], [0, 0]]
    two, _, _ = tables(cases, control, 5, max_count=2)
    assert two.tolist() == [[0, 0, 2], [0, 0, 1], [0, 1, 0], [0, 1, 1], [0, 2, 0]]
    assert np.array_equal(tables(cases, control, 5, max_count=3)[0], carriers) and np.array_equal(tables(cases, control, 5, max_count=9)[0], carriers)


def test_invariants_on_the_reference(gen):
    """Invariants 2 - 4 and 7 on the reference itself, and the lists as sets."""
    rng = np.random.default_rng(5)
    ind, fa, mo, _ = random_pedigree(rng, 300, p_founder=0.08, p_one_parent=0.1, p_selfing=0.05, max_back=25)
    cases = rng.choice(ind[100:], size=14, replace=False).astype(np.int64)
    cases[9], cases[13], cases[4] = cases[1], cases[1], ind[0]
    controls = np.setdiff1d(ind[60:], cases)[::23][:8]
    S = 1000
    plain = CarryVector(ind, fa, mo, cases, None, S, 31)
    carriers, homozygotes, excluded = plain.at(S)
    assert plain.n == 12 and carriers.shape == (plain.n_labels, 13)
    assert check_invariants(carriers, homozygotes, excluded, plain.alleles, S, cases) >= 2
    assert np.any(homozygotes[:, 1:]) and np.any(carriers[:, 3:])
    ref = CarryVector(ind, fa, mo, cases, controls, S, 31)
    c2, h2, x2 = ref.at(S)
    check_invariants(c2, h2, x2, ref.alleles, S, cases, controls)
    assert np.any((x2 > 0) & (x2 < S))
    key = {(int(a), int(s)): k for k, (a, s) in enumerate(ref.alleles.tolist())}
    at = np.array([key[(int(a), int(s))] for a, s in plain.alleles.tolist()])            # 7: the table with controls holds every allele of the one without
    assert np.all(c2[at][:, 1:] <= carriers[:, 1:]) and np.all(h2[at][:, 1:] <= homozygotes[:, 1:]) and np.any(c2[at][:, 1:] < carriers[:, 1:])
    other = CarryVector(ind, fa, mo, np.concatenate([cases[::-1], cases[:5]]), np.concatenate([controls, controls[::-1]]), S, 31)
    for a, b in zip(other.at(S), (c2, h2, x2)):
        assert np.array_equal(a, b)
    for a, b in zip(ref.at(S, max_count=2), (c2, h2, x2)):
        assert a.shape == (b.shape[0], 3)[: a.ndim] and np.array_equal(a[..., :2], b[..., :2])
        assert a.ndim == 1 or np.array_equal(a[:, 2], b[:, 2:].sum(axis=1))


def _check_plan(gen, ind, fa, mo, cases, controls, **kw):
    h = gen.CarriersPlan(ind, fa, mo, cases, controls, simul_no=64, seed=1, **kw)
    g = gen.IdentityPlan(ind, fa, mo, np.concatenate([cases, controls]).astype(np.int64), simul_no=64, seed=1)
    try:
        assert (h.n_live, h.levels, h.n_labels, h.planes, h.n_pro) == (g.n_live, g.levels, g.n_labels, g.planes, g.n_pro)
        assert np.array_equal(h.rows_per_level(), g.rows_per_level())
        got = h.alleles()
        assert got.dtype == np.int64 and np.array_equal(got, g.alleles())
        st, gs = h.stats(), g.stats()
        assert st["sweep_ms"] == 0.0 and st["count_ms"] == 0.0 and st["count_bytes"] == 0.0
        assert (st["planes"], st["levels"], st["panel_cols"], st["panels"]) == (gs["planes"], gs["levels"], gs["panel_cols"], gs["panels"])
        assert (st["n_cases"], st["n_controls"]) == (len(np.unique(cases)), len(np.unique(controls))) == (h.n_cases, h.n_controls)
        return h.n_labels, st
    finally:
        h.close()
        g.close()


def test_plan_is_the_identity_plan_on_cases_and_controls(gen):
    ped = gen.genealogy(gen.geneaJi)
    pro = gen.pro(ped)
    n_labels, st = _check_plan(gen, ped.ind, ped.father, ped.mother, pro, np.zeros(0, dtype=np.int64))
    assert (st["chunk_labels"], st["chunks"], st["lds_bytes"], st["columns"]) == (n_labels, 1, 256 * (n_labels | 1), len(pro) + 1)
    _check_plan(gen, ped.ind, ped.father, ped.mother, pro[[2, 0, 2]], pro[[1, 1]])
    rng = np.random.default_rng(99)
    seen = set()
    for k in range(60):
        ind, fa, mo, _ = random_pedigree(rng, int(rng.integers(2, 400)), p_founder=0.15, p_one_parent=0.1, p_selfing=0.03, max_back=40)
        order = rng.permutation(ind)
        n_cases = int(rng.integers(1, min(10, len(ind))))
        cases = rng.choice(order[:n_cases], size=n_cases + int(rng.integers(0, 3)), replace=True).astype(np.int64)
        rest = order[n_cases:]
        controls = rng.choice(rest, size=int(rng.integers(0, 6)), replace=True).astype(np.int64) if k % 3 else rest[:0]
        arg, mc = [0, 32, 33, 64][k % 4], [0, 1, 2, 100][k % 4]
        n_labels, st = _check_plan(gen, ind, fa, mo, cases, controls, chunk_labels=arg, max_count=mc)
        lc = min(n_labels, (arg + 31) // 32 * 32 if arg else 608)
        n = len(np.unique(cases))
        assert (st["chunk_labels"], st["chunks"], st["lds_bytes"]) == (lc, -(-n_labels // lc), 256 * (lc | 1))
        assert st["columns"] == (min(n, mc) if mc else n) + 1
        seen.add(st["chunks"])
    assert len(seen) >= 3


def test_planned_shapes(gen):
    h = gen.CarriersPlan(IND, FA, MO, [8, 6, 8], [9, 9], simul_no=5000, seed=3, panel_cols=1000, chunk_labels=1, max_count=1)
    try:
        assert (h.n_live, h.levels, h.n_labels, h.planes, h.n_pro, h.simul_no, h.seed) == (9, 4, 7, 3, 5, 5000, 3)
        assert h.alleles().tolist() == [[1, 0], [1, 1], [2, 0], [2, 1], [7, 0], [9, 0], [9, 1]]
        assert (h.n_cases, h.n_controls, h.columns) == (2, 1, 2)
        st = h.stats()
        assert (st["panel_cols"], st["panels"], st["chunk_labels"], st["chunks"], st["lds_bytes"]) == (1024, 5, 7, 1, 256 * 7)
    finally:
        h.close()


def test_argument_errors(gen):
    ok = dict(case_ids=[8, 6], control_ids=[9], simul_no=10, seed=3)

    def plan(**kw):
        a = {**ok, **kw}
        gen.CarriersPlan(a.pop("ind", IND), a.pop("fa", FA), a.pop("mo", MO), **a).close()

    plan()
    plan(control_ids=None)
    plan(control_ids=[])
    plan(simul_no=1 << 24)
    plan(simul_no=1, panel_cols=7, chunk_labels=7, max_count=7)
    plan(chunk_labels=2**31 - 1, max_count=2**31 - 1)
    plan(case_ids=[8, 8, 6], control_ids=[9, 9, 7])
    with pytest.raises(KeyError):
        plan(case_ids=[8, 99])
    with pytest.raises(KeyError):
        plan(control_ids=[99])
    with pytest.raises(KeyError):
        plan(case_ids=[0])
    for kw in (dict(simul_no=0), dict(simul_no=-5), dict(simul_no=(1 << 24) + 1), dict(case_ids=[]), dict(case_ids=[], control_ids=[]), dict(panel_cols=-1),
               dict(chunk_labels=-1), dict(max_count=-1)):
        with pytest.raises(ValueError):
            plan(**kw)
    for cases, controls in (([8, 6], [6]), ([8, 6], [9, 8, 9]), ([1], [1]), ([8, 6, 8], [7, 6])):
        with pytest.raises(ValueError, match="as a case and as a control"):
            plan(case_ids=cases, control_ids=controls)
    with pytest.raises(Exception, match="duplicate"):
        plan(ind=np.array([1, 2, 3, 4, 5, 6, 7, 8, 1]))
    with pytest.raises(Exception, match="rank order"):
        plan(fa=np.array([8, 0, 1, 1, 3, 3, 0, 5, 0]))
    # the C entry point itself: NULL out, NULL lists, negative sizes, NULL handles
    L = gen._capi.lib()
    i64 = ctypes.POINTER(ctypes.c_int64)
    pro, con = np.array([8], dtype=np.int64), np.array([9], dtype=np.int64)
    ped = [len(IND), IND.ctypes.data_as(i64), FA.ctypes.data_as(i64), MO.ctypes.data_as(i64)]
    h = ctypes.c_void_p()
    ARG = gen._capi.GENPHI_ERR_ARG
    assert L.genphi_carry_create(*ped, 1, pro.ctypes.data_as(i64), 1, con.ctypes.data_as(i64), 10, 3, 0, 0, 0, None) == ARG
    assert L.genphi_carry_create(*ped, 1, pro.ctypes.data_as(i64), 1, None, 10, 3, 0, 0, 0, ctypes.byref(h)) == ARG and not h.value
    assert L.genphi_carry_create(*ped, 1, None, 0, None, 10, 3, 0, 0, 0, ctypes.byref(h)) == ARG and not h.value
    assert L.genphi_carry_create(*ped, -1, pro.ctypes.data_as(i64), 0, None, 10, 3, 0, 0, 0, ctypes.byref(h)) == ARG and not h.value
    assert L.genphi_carry_create(*ped, 1, pro.ctypes.data_as(i64), -1, con.ctypes.data_as(i64), 10, 3, 0, 0, 0, ctypes.byref(h)) == ARG and not h.value
    assert L.genphi_carry_create(*ped, 1, pro.ctypes.data_as(i64), 0, None, 10, 3, 0, 0, 0, ctypes.byref(h)) == 0 and h.value
    L.genphi_carry_destroy(h)
    assert L.genphi_carry_levels(None, None, None, None) == ARG and L.genphi_carry_alleles(None, None, None, None, None) == ARG
    assert L.genphi_carry_compute(None, 0) == ARG
    assert L.genphi_carry_stats(None, *([None] * 14)) == ARG
    for name in ("carriers", "homozygotes", "excluded"):
        assert getattr(L, "genphi_carry_%s_to_host" % name)(None, None) == ARG
    L.genphi_carry_destroy(None)
    hp = gen.CarriersPlan(IND, FA, MO, [8, 6], simul_no=10, seed=3)
    for fn in (hp.carriers_to_host, hp.homozygotes_to_host, hp.excluded_to_host):
        with pytest.raises(ValueError, match="nothing computed"):
            fn()
    hp.close()
    ped = _ped(gen, IND, FA, MO)
    with pytest.raises(ValueError):
        gen.simuCarriers(ped, pro=[])
    with pytest.raises(KeyError):
        gen.simuCarriers(ped, pro=[77])
    with pytest.raises(KeyError):
        gen.simuCarriers(ped, pro=[8], controls=[77])
    with pytest.raises(ValueError):
        gen.simuCarriers(ped, pro=[8, 6], controls=[6])
    with pytest.raises(ValueError):
        gen.simuCarriers(ped, simulNo=0)
    with pytest.raises(ValueError):
        gen.simuCarriers(ped, maxCount=-1)
    with pytest.raises(TypeError):
        gen.simuCarriers(ped, ancestors=[1])
    h1, h2 = gen.CarriersPlan(IND, FA, MO, [8]), gen.CarriersPlan(IND, FA, MO, [8])
    assert 0 <= h1.seed < 2**64 and h1.seed != h2.seed and h1.simul_no == 5000
    h1.close()
    h2.close()


def test_the_limits_on_unrelated_founders(gen):
    """n = 32,767 distinct cases are taken and 32,768 refused; repeats do not count.  With 32,767 founder cases the tables have
    2 x 32,767 x 32,768 = 2^31 - 65,536 cells: one founder control adds 65,536 and passes 2^31 - 1, unless max_count narrows W."""
    ind, fa, mo = _founders(32780)
    h = gen.CarriersPlan(ind, fa, mo, ind[:32767], simul_no=64, seed=1)
    try:
        assert (h.n_cases, h.n_controls, h.columns, h.n_labels, h.planes) == (32767, 0, 32768, 65534, 16)
        assert h.n_labels * h.columns == 2**31 - 65536
        st = h.stats()
        assert (st["chunk_labels"], st["chunks"], st["lds_bytes"]) == (608, 108, 155904)                # the default chunk is the widest
    finally:
        h.close()
    gen.CarriersPlan(ind, fa, mo, np.concatenate([ind[:32767], ind[:40]]), simul_no=64, seed=1, max_count=5).close()
    with pytest.raises(ValueError, match="32,767"):
        gen.CarriersPlan(ind, fa, mo, ind[:32768], simul_no=64, seed=1)
    with pytest.raises(ValueError, match="32,767"):
        gen.CarriersPlan(ind, fa, mo, ind[:32768], simul_no=64, seed=1, max_count=1)
    for n_controls in (1, 3):
        with pytest.raises(ValueError, match="cells"):
            gen.CarriersPlan(ind, fa, mo, ind[:32767], ind[32767:32767 + n_controls], simul_no=64, seed=1)
    with pytest.raises(ValueError, match="cells"):
        gen.CarriersPlan(ind, fa, mo, ind[:32767], ind[32767:32770], simul_no=64, seed=1, max_count=32766)
    h = gen.CarriersPlan(ind, fa, mo, ind[:32767], ind[32767:32770], simul_no=64, seed=1, max_count=32765)
    try:
        assert (h.n_controls, h.columns, h.n_labels) == (3, 32766, 65540) and h.n_labels * h.columns == 2**31 - 8
    finally:
        h.close()


def test_symbols_are_exported_declared_and_bound(gen):
    from genlib_jl_amd import _capi
    header = open(os.path.join(ROOT, "include", "genphi.h")).read()
    L = ctypes.CDLL(_capi.LIB_PATH)
    names = ["genphi_carry_" + n for n in ("create", "levels", "alleles", "compute", "carriers_to_host", "homozygotes_to_host", "excluded_to_host", "stats",
                                           "destroy")]
    for name in names:
        assert hasattr(L, name) and name in _capi.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, header), name
    assert sum(n.startswith("genphi_carry_") for n in _capi.EXPORTED_SYMBOLS) == 9
    assert len(_capi.lib().genphi_carry_create.argtypes) == 14 and len(_capi.lib().genphi_carry_stats.argtypes) == 15
    assert gen.CarriersPlan is _capi.CarriersPlan and gen.simuCarriers.__doc__ and gen.SimuCarriers.__doc__
    text = header[header.index("gen.simuCarriers"):header.index("typedef struct genphi_carry")]
    for k in range(1, 8):
        assert re.search(r"^ \*\s+%d\. " % k, text, re.M), k
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"carry.hip"' in entry and '"carry.h"' in entry


def test_SimuCarriers_shares(gen):
    """The shares from hand-made integer tables, S = 10, three cases: founder 10 (two alleles), half-founder 20, founder 30."""
    alleles = np.array([[10, 0], [10, 1], [20, 1], [30, 0], [30, 1]], dtype=np.int64)
    carriers = np.array([[2, 3, 1, 4], [5, 0, 1, 4], [7, 1, 0, 0], [10, 0, 0, 0], [1, 2, 6, 1]], dtype=np.int32)
    homozygotes = np.array([[8, 1, 0, 1], [10, 0, 0, 0], [8, 0, 0, 0], [10, 0, 0, 0], [8, 2, 0, 0]], dtype=np.int32)
    excluded = np.array([0, 0, 2, 0, 0], dtype=np.int32)
    r = gen.SimuCarriers(np.array([7, 8, 9]), np.array([5]), alleles, carriers, homozygotes, excluded, 10, 1)
    assert not r.lumped and r.founders.tolist() == [10, 20, 30]
    assert r.at_least(1).dtype == np.float64 and r.at_least(1).tolist() == [0.8, 0.5, 0.1, 0.0, 0.9]
    assert r.at_least(0).tolist() == [1.0, 1.0, 0.8, 1.0, 1.0] and r.at_least(3).tolist() == [0.4, 0.4, 0.0, 0.0, 0.1] and r.at_least(4).tolist() == [0.0] * 5
    assert r.at_least(1, homozygous=True).tolist() == [0.2, 0.0, 0.0, 0.0, 0.2]
    assert r.mean_carriers.tolist() == [17 / 10, 14 / 10, 1 / 10, 0.0, 17 / 10]
    assert r.prob_all.tolist() == [0.4, 0.4, 0.0, 0.0, 0.1] and r.prob_all_hom.tolist() == [0.1, 0.0, 0.0, 0.0, 0.0]
    assert r.posterior.tolist() == [4 / 9, 4 / 9, 0.0, 0.0, 1 / 9] and r.ranking.tolist() == [0, 1, 4, 2, 3]
    assert "3 cases" in repr(r) and "1 controls" in repr(r) and "5 founder alleles" in repr(r)
    with pytest.raises(ValueError):
        r.at_least(-1)
    none = gen.SimuCarriers(np.array([7, 8, 9]), np.zeros(0, dtype=np.int64), alleles, carriers * np.array([1, 1, 1, 0], dtype=np.int32), homozygotes, excluded, 10, 1)
    assert none.posterior.tolist() == [0.0] * 5 and none.ranking.tolist() == [0, 1, 2, 3, 4]
    cut = gen.SimuCarriers(np.array([7, 8, 9, 11]), np.array([5]), alleles, carriers, homozygotes, excluded, 10, 1)      # four cases, columns 0 .. 3
    assert cut.lumped and cut.prob_all is None and cut.prob_all_hom is None and cut.posterior is None and cut.ranking is None and cut.mean_carriers is None
    assert cut.at_least(3).tolist() == [0.4, 0.4, 0.0, 0.0, 0.1]
    with pytest.raises(ValueError):
        cut.at_least(4)


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_carry_h_as_a_stand_alone_program(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "carry_check")
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra"] + flags + [os.path.join(ROOT, "tests", "carry_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if san is not None and build.returncode != 0 and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("this toolchain has no -fsanitize=" + san)
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    if san is not None and run.returncode != 0 and not run.stdout and any(
            t in run.stderr for t in ("unexpected memory mapping", "runtime does not come first", "failed to intercept", "ReserveShadowMemoryRange failed")):
        pytest.skip("the sanitizer runtime does not start in this environment: " + run.stderr[:200])
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    m = SUMMARY.search(run.stdout)
    assert m, run.stdout[-1500:]
    cases, walked, plans, overlaps, repeats, violations = (int(v) for v in m.groups())
    assert violations == 0 and cases >= 250 and walked > 10**7 and plans == 20000 and overlaps > 1000 and repeats > 1000
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
