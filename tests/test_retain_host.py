"""gen.simuRetention without a GPU: the invariants of the definition (include/genphi.h, genphi_retain_*) on the reference of
tests/retain_oracle.py, the host plan of gen.RetentionPlan against gen.IdentityPlan's, every argument error, a proband list that
gen.IdentityPlan refuses, the shares of gen.SimuRetention from hand-made integers, and csrc/retain.h as a stand-alone program
under AddressSanitizer + UndefinedBehaviorSanitizer (tests/retain_check.cpp)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from ident_oracle import IdentVector
from random_pedigree import random_pedigree
from retain_oracle import RetainVector, check_invariants, presence, reductions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genlib.jl_amd", "csrc")

SUMMARY = re.compile(r"^retain check: (\d+) chunk cases, (\d+) chunks walked, (\d+) borders with a halo, (\d+) plans, (\d+) panels fit, (\d+) narrowed, "
                     r"(\d+) refused; (\d+) violations$", re.M)


def _args(ped):
    return ped.ind, ped.father, ped.mother


def _ped(gen, ind, fa, mo):
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)


def _by_allele(alleles, values):
    return {(int(a), int(s)): int(v) for (a, s), v in zip(alleles.tolist(), values.tolist())}


def _mixed():
    """300 individuals with half-founders and selfing; 14 probands, two of them repeats, one a founder, some with children."""
    rng = np.random.default_rng(5)
    ind, fa, mo, _ = random_pedigree(rng, 300, p_founder=0.08, p_one_parent=0.1, p_selfing=0.05, max_back=25)
    pro = rng.choice(ind[100:], size=14, replace=False).astype(np.int64)
    pro[9], pro[13], pro[4] = pro[1], pro[1], ind[0]
    return ind, fa, mo, pro


@pytest.fixture(scope="module", params=["geneaJi", "random"])
def case(request, gen):
    if request.param == "geneaJi":
        ped = gen.genealogy(gen.geneaJi)
        ind, fa, mo, pro = ped.ind, ped.father, ped.mother, gen.pro(ped)
    else:
        ind, fa, mo, pro = _mixed()
    return ind, fa, mo, pro, RetainVector(ind, fa, mo, pro, 5000, 31)


def test_the_oracle_on_hand_made_labels():
    """Three probands, five labels (founder 10: labels 0, 1; half-founder 20: label 2; founder 30: labels 3, 4), four simulations."""
    alleles = np.array([[10, 0], [10, 1], [20, 1], [30, 0], [30, 1]])
    labels = np.array([[[0, 0, 1, 3], [1, 0, 1, 4]],
                       [[2, 0, 1, 3], [1, 1, 1, 3]],
                       [[0, 4, 1, 3], [0, 3, 1, 3]]], dtype=np.int32)
    table = presence(labels, 5)
    assert table.astype(int).tolist() == [[1, 1, 0, 0], [1, 1, 1, 0], [1, 0, 0, 0], [0, 1, 0, 1], [0, 1, 0, 1]]
    survived, both, distinct = reductions(labels, alleles)
    assert survived.tolist() == [2, 3, 1, 2, 2] and both.tolist() == [2, 0, 0, 2, 0] and distinct.tolist() == [3, 4, 1, 2]
    assert check_invariants(survived, both, distinct, alleles, 4, [1, 2, 3]) == 0


def test_invariants_on_the_reference(gen, case):
    ind, fa, mo, pro, ref = case
    S = 5000
    survived, both, distinct = ref.at(S)
    listed_founder_sides = check_invariants(survived, both, distinct, ref.alleles, S, pro)                  # 1 - 4
    if len(ind) == 300:
        assert listed_founder_sides >= 2 and np.any((both > 0) & (both < survived))
    # 5: order and repeats of the list change nothing
    rng = np.random.default_rng(8)
    for other in (np.unique(pro), rng.permutation(pro), np.concatenate([pro, pro[:3], pro[::-1]])):
        r2 = RetainVector(ind, fa, mo, other, S, 31)
        assert np.array_equal(r2.alleles, ref.alleles)
        for a, b in zip(r2.at(S), (survived, both, distinct)):
            assert np.array_equal(a, b)
    # 7: the prefix rule, and another seed
    for s in (64, 129):
        assert np.array_equal(RetainVector(ind, fa, mo, pro, s, 31).at(s)[2], distinct[:s])
        assert np.array_equal(ref.at(s)[2], distinct[:s])
    assert not np.array_equal(RetainVector(ind, fa, mo, pro, 129, 32).at(129)[2], distinct[:129])
    # 8: gen.branching(ped, pro=P) first changes nothing
    pruned = gen.branching(_ped(gen, ind, fa, mo), pro=pro)
    r3 = RetainVector(pruned.ind, pruned.father, pruned.mother, pro, S, 31)
    assert np.array_equal(r3.alleles, ref.alleles)
    for a, b in zip(r3.at(S), (survived, both, distinct)):
        assert np.array_equal(a, b)
    # 9: a sub-list against its superset, matched through (ID, side)
    sub = np.unique(pro)[::2]
    r4 = RetainVector(ind, fa, mo, sub, S, 31)
    big, small = _by_allele(ref.alleles, survived), _by_allele(r4.alleles, r4.at(S)[0])
    assert set(small) <= set(big) and all(small[k] <= big[k] for k in small)
    if len(ind) == 300:
        assert len(small) < len(big) and any(small[k] < big[k] for k in small)


def _check_plan(gen, ind, fa, mo, pro, **kw):
    h = gen.RetentionPlan(ind, fa, mo, pro, simul_no=64, seed=1, **kw)
    g = gen.IdentityPlan(ind, fa, mo, pro, simul_no=64, seed=1)
    try:
        assert (h.n_live, h.levels, h.n_labels, h.planes, h.n_pro) == (g.n_live, g.levels, g.n_labels, g.planes, g.n_pro)
        assert np.array_equal(h.rows_per_level(), g.rows_per_level())
        got = h.alleles()
        assert got.dtype == np.int64 and np.array_equal(got, g.alleles())
        st, gs = h.stats(), g.stats()
        assert st["sweep_ms"] == 0.0 and st["mark_ms"] == 0.0 and st["mark_bytes"] == 0.0
        assert (st["planes"], st["levels"], st["panel_cols"], st["panels"], st["lanes_per_row"]) == (
            gs["planes"], gs["levels"], gs["panel_cols"], gs["panels"], gs["lanes_per_row"])
        return h.n_labels, st
    finally:
        h.close()
        g.close()


def test_plan_is_the_identity_plan(gen):
    ped = gen.genealogy(gen.geneaJi)
    n_labels, st = _check_plan(gen, *_args(ped), gen.pro(ped))
    assert (st["chunk_labels"], st["chunks"], st["lds_bytes"]) == (n_labels, 1, 256)
    _check_plan(gen, *_args(ped), gen.pro(ped)[[2, 0, 2]])
    _check_plan(gen, *_args(ped), ped.ind)
    rng = np.random.default_rng(99)
    seen = set()
    for k in range(60):
        ind, fa, mo, _ = random_pedigree(rng, int(rng.integers(1, 400)), p_founder=0.15, p_one_parent=0.1, p_selfing=0.03, max_back=40)
        pro = rng.choice(ind, size=int(rng.integers(1, 10)), replace=True).astype(np.int64)
        arg = [0, 32, 33, 64][k % 4]
        n_labels, st = _check_plan(gen, ind, fa, mo, pro, chunk_labels=arg)
        lc = min(n_labels, (arg + 31) // 32 * 32) if arg else n_labels
        stride = (lc // 32 + 1) | 1
        assert (st["chunk_labels"], st["chunks"], st["lds_bytes"]) == (lc, -(-n_labels // lc), 256 * stride)
        seen.add(st["chunks"])
    assert len(seen) >= 3


def test_planned_shapes(gen):
    ind = np.arange(1, 10, dtype=np.int64)
    fa = np.array([0, 0, 1, 1, 3, 3, 0, 5, 0], dtype=np.int64)
    mo = np.array([0, 0, 2, 2, 4, 3, 4, 7, 0], dtype=np.int64)
    h = gen.RetentionPlan(ind, fa, mo, [8, 6, 8], simul_no=5000, seed=3, panel_cols=1000, chunk_labels=1)
    try:
        assert (h.n_live, h.levels, h.n_labels, h.planes, h.n_pro, h.simul_no, h.seed) == (8, 4, 5, 3, 3, 5000, 3)
        assert h.alleles().tolist() == [[1, 0], [1, 1], [2, 0], [2, 1], [7, 0]]
        st = h.stats()
        assert (st["panel_cols"], st["panels"], st["lanes_per_row"], st["chunk_labels"], st["chunks"], st["lds_bytes"]) == (1024, 5, 8, 5, 1, 256)
    finally:
        h.close()


def test_argument_errors(gen):
    ind = np.arange(1, 10, dtype=np.int64)
    fa = np.array([0, 0, 1, 1, 3, 3, 0, 5, 0], dtype=np.int64)
    mo = np.array([0, 0, 2, 2, 4, 3, 4, 7, 0], dtype=np.int64)
    ok = dict(pro_ids=[8, 6], simul_no=10, seed=3)

    def plan(**kw):
        a = {**ok, **kw}
        gen.RetentionPlan(a.pop("ind", ind), a.pop("fa", fa), a.pop("mo", mo), **a).close()

    plan()
    plan(simul_no=1 << 24)
    plan(simul_no=1, panel_cols=7, chunk_labels=7, mark="or")
    plan(mark="test", chunk_labels=2**31 - 1)
    with pytest.raises(KeyError):
        plan(pro_ids=[8, 99])
    with pytest.raises(KeyError):
        plan(pro_ids=[0])
    for kw in (dict(simul_no=0), dict(simul_no=-5), dict(simul_no=(1 << 24) + 1), dict(pro_ids=[]), dict(panel_cols=-1), dict(chunk_labels=-1),
               dict(mark="both"), dict(mark=1)):
        with pytest.raises(ValueError):
            plan(**kw)
    with pytest.raises(Exception, match="duplicate"):
        plan(ind=np.array([1, 2, 3, 4, 5, 6, 7, 8, 1]))
    with pytest.raises(Exception, match="rank order"):
        plan(fa=np.array([8, 0, 1, 1, 3, 3, 0, 5, 0]))
    # the C entry point itself: an unknown flag, both forms at once, NULL out, NULL handles
    L = gen._capi.lib()
    i64 = ctypes.POINTER(ctypes.c_int64)
    pro = np.array([8], dtype=np.int64)
    a = [len(ind), ind.ctypes.data_as(i64), fa.ctypes.data_as(i64), mo.ctypes.data_as(i64), 1, pro.ctypes.data_as(i64), 10, 3, 0, 0]
    h = ctypes.c_void_p()
    ARG = gen._capi.GENPHI_ERR_ARG
    assert L.genphi_retain_create(*a, 4, ctypes.byref(h)) == ARG and not h.value
    assert L.genphi_retain_create(*a, 3, ctypes.byref(h)) == ARG and not h.value
    assert L.genphi_retain_create(*a, 0, None) == ARG
    assert L.genphi_retain_levels(None, None, None, None) == ARG and L.genphi_retain_alleles(None, None, None, None, None) == ARG
    assert L.genphi_retain_compute(None, 0) == ARG
    assert L.genphi_retain_stats(None, *([None] * 12)) == ARG
    for name in ("survived", "both", "distinct"):
        assert getattr(L, "genphi_retain_%s_to_host" % name)(None, None) == ARG
    L.genphi_retain_destroy(None)
    hp = gen.RetentionPlan(ind, fa, mo, [8, 6], simul_no=10, seed=3)
    for fn in (hp.survived_to_host, hp.both_to_host, hp.distinct_to_host):
        with pytest.raises(ValueError, match="nothing computed"):
            fn()
    hp.close()
    ped = _ped(gen, ind, fa, mo)
    with pytest.raises(ValueError):
        gen.simuRetention(ped, pro=[])
    with pytest.raises(KeyError):
        gen.simuRetention(ped, pro=[77])
    with pytest.raises(ValueError):
        gen.simuRetention(ped, simulNo=0)
    with pytest.raises(TypeError):
        gen.simuRetention(ped, probSurvival=1.0)
    h1, h2 = gen.RetentionPlan(ind, fa, mo, [8]), gen.RetentionPlan(ind, fa, mo, [8])
    assert 0 <= h1.seed < 2**64 and h1.seed != h2.seed and h1.simul_no == 5000
    h1.close()
    h2.close()


def test_a_list_that_the_identity_plan_refuses(gen):
    """50,000 probands: 2.5 x 10^9 ordered pairs.  100 founders, and every proband a child of two of them."""
    n_f, n = 100, 50000
    k = np.arange(n, dtype=np.int64)
    ind = np.concatenate([np.arange(1, n_f + 1, dtype=np.int64), n_f + 1 + k])
    fa = np.concatenate([np.zeros(n_f, dtype=np.int64), 1 + k % 50])
    mo = np.concatenate([np.zeros(n_f, dtype=np.int64), 51 + (k // 50) % 50])
    pro = ind[n_f:]
    with pytest.raises(ValueError, match="ordered pairs"):
        gen.IdentityPlan(ind, fa, mo, pro, simul_no=5000, seed=1)
    h = gen.RetentionPlan(ind, fa, mo, pro, simul_no=5000, seed=1)
    try:
        assert (h.n_pro, h.n_live, h.levels, h.n_labels, h.planes) == (n, n + n_f, 2, 2 * n_f, 8)
        assert h.rows_per_level().tolist() == [n_f, n]
        st = h.stats()
        assert (st["chunk_labels"], st["chunks"], st["panel_cols"], st["panels"]) == (200, 1, 5120, 1)
    finally:
        h.close()


def test_symbols_are_exported_declared_and_bound(gen):
    from genlib_jl_amd import _capi
    header = open(os.path.join(ROOT, "include", "genphi.h")).read()
    L = ctypes.CDLL(_capi.LIB_PATH)
    names = ["genphi_retain_" + n for n in ("create", "levels", "alleles", "compute", "survived_to_host", "both_to_host", "distinct_to_host", "stats",
                                            "destroy")]
    for name in names:
        assert hasattr(L, name) and name in _capi.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, header), name
    assert sum(n.startswith("genphi_retain_") for n in _capi.EXPORTED_SYMBOLS) == 9
    assert len(_capi.lib().genphi_retain_create.argtypes) == 12 and len(_capi.lib().genphi_retain_stats.argtypes) == 13
    for macro, value in (("GENPHI_RETAIN_FLAG_PLAIN_OR", 1), ("GENPHI_RETAIN_FLAG_TEST_FIRST", 2)):
        assert re.search(r"#define %s %d\b" % (macro, value), header) and getattr(_capi, macro) == value
    assert gen.RetentionPlan is _capi.RetentionPlan and gen.simuRetention.__doc__ and gen.SimuRetention.__doc__
    for k in range(1, 11):
        assert re.search(r"^ \*\s+%d\. " % k, header[header.index("gen.simuRetention"):header.index("GENPHI_RETAIN_FLAG_PLAIN_OR 1")], re.M), k


def test_SimuRetention_shares(gen):
    """The shares from hand-made integers, S = 10: founder 10 (two alleles), half-founder 20 (one, never kept), founder 30 (two, one of
    them never kept), half-founder 40 (one)."""
    alleles = np.array([[10, 0], [10, 1], [20, 1], [30, 0], [30, 1], [40, 0]], dtype=np.int64)
    survived = np.array([8, 6, 0, 10, 0, 5], dtype=np.int32)
    both = np.array([5, 0, 0, 0, 0, 0], dtype=np.int32)
    distinct = np.array([3, 3, 3, 3, 3, 3, 3, 3, 3, 2], dtype=np.int32)
    p = np.array([0.25, 0.25, 0.125, 0.125, 0.125, 0.125])
    r = gen.SimuRetention(np.array([7, 8]), alleles, survived, both, distinct, 10, 1, p)
    assert r.retention.dtype == np.float64 and r.retention.tolist() == [0.8, 0.6, 0.0, 1.0, 0.0, 0.5]
    assert r.founders.tolist() == [10, 20, 30, 40] and r.n_alleles.tolist() == [2, 1, 2, 1]
    assert r.kept.tolist() == [14 / 20, 0.0, 10 / 20, 5 / 10]
    assert r.lost.tolist() == [(10 - 9) / 10, 1.0, 0.0, 0.5]
    assert r.whole[[0, 2]].tolist() == [0.5, 0.0] and np.isnan(r.whole[[1, 3]]).all()
    assert r.alleles_mean == 29 / 10 and r.hist.tolist() == [0, 0, 1, 9]
    assert r.alleles_sd == np.sqrt(10 * 85 - 29 * 29) / 10
    assert p.sum() == 1.0 and r.fe == 1 / (2 * (2 / 16 + 4 / 64)) and r.fg_dropped == 2
    assert r.fg == 1 / (2 * float(np.sum([p[0] ** 2 * (10 / 8), p[1] ** 2 * (10 / 6), p[3] ** 2 * (10 / 10), p[5] ** 2 * (10 / 5)])))
    assert r.fe >= r.fg and "2 probands" in repr(r) and "6 founder alleles" in repr(r)
    q = gen.SimuRetention(np.array([7]), alleles, survived, both, distinct, 10, 1)
    assert q.p is None and q.fe is None and q.fg is None and q.fg_dropped == 2


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_retain_h_as_a_stand_alone_program(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "retain_check")
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra"] + flags + [os.path.join(ROOT, "tests", "retain_check.cpp"), "-o", exe]
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
    cases, walked, halos, plans, fits, narrowed, refused, violations = (int(v) for v in m.groups())
    assert violations == 0 and cases >= 150 and walked > 10**6 and halos > 10**6 and plans == 20000 and min(fits, narrowed, refused) > 1000
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
