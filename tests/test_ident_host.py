"""gen.simuIdentity without a GPU: the two CPU references of tests/ident_oracle.py against each other, the invariants of the
definition (include/genphi.h) on the reference, the host plan of gen.IdentityPlan (live rows, levels, allele table, B, argument
errors) against the vectorised reference, the plan as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/ident_plan_check.cpp), and the kinship estimate of the reference against the exact kinship."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from exact_kinship import ExactKinship
from ident_oracle import IdentVector, counts_of, ident_literal, kinship_of, state_of, swap_roles
from random_pedigree import random_pedigree
from simu_oracle import SimuVector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genlib.jl_amd", "csrc")
DATA = os.path.join(ROOT, "genlib.jl_amd", "data")

SUMMARY = re.compile(r"^ident plan check: (\d+) pedigrees, (\d+) rows, (\d+) labels, (\d+) half-founders, (\d+) selfings, (\d+) lists with repeats, "
                     r"(\d+) refusals, most planes (\d+), most levels (\d+); (\d+) violations$", re.M)


def _args(ped):
    return ped.ind, ped.father, ped.mother


def random_case(rng, n):
    """A random pedigree of n individuals (half-founders, selfing) with probands anywhere in it, repeats included."""
    ind, fa, mo, _ = random_pedigree(rng, n, p_founder=0.15, p_one_parent=0.1, p_selfing=0.03, max_back=40)
    pro = rng.choice(ind, size=int(rng.integers(1, 10)), replace=True).astype(np.int64)
    return ind, fa, mo, pro


def shapes_pedigree():
    """1, 2 founders; 3 = (1, 2); 4 = (1, 2); 5 = (3, 4) inbred; 6 = (3, 3) selfed; 7 = (0, 4) half-founder; 8 = (5, 7); 9 founder."""
    ind = np.arange(1, 10, dtype=np.int64)
    fa = np.array([0, 0, 1, 1, 3, 3, 0, 5, 0], dtype=np.int64)
    mo = np.array([0, 0, 2, 2, 4, 3, 4, 7, 0], dtype=np.int64)
    return ind, fa, mo


def test_states_partition_the_label_patterns():
    """state_of on every pattern of four labels out of four: each of the nine states occurs, and exchanging the two individuals
    exchanges 3 <-> 5 and 4 <-> 6."""
    seen = set()
    swap = {1: 1, 2: 2, 3: 5, 4: 6, 5: 3, 6: 4, 7: 7, 8: 8, 9: 9}
    for a in range(4):
        for b in range(4):
            for c in range(4):
                for d in range(4):
                    s = state_of(a, b, c, d)
                    seen.add(s)
                    assert state_of(c, d, a, b) == swap[s] and state_of(b, a, d, c) == s
    assert seen == set(range(1, 10))
    lab = np.array([[[a], [b]] for a in range(4) for b in range(4)], dtype=np.int32)           # 16 "probands", one simulation
    c = counts_of(lab)
    for i in range(16):
        for j in range(16):
            assert c[i, j].sum() == 1 and c[i, j, state_of(*lab[i, :, 0], *lab[j, :, 0]) - 1] == 1


def test_oracles_agree_on_geneaJi(gen):
    ped = gen.genealogy(gen.geneaJi)
    pro = gen.pro(ped)
    labels, counts, alleles = ident_literal(*_args(ped), pro, 130, 11)
    o = IdentVector(*_args(ped), pro)
    assert np.array_equal(labels, o.labels(130, 11)) and np.array_equal(counts, o.counts(130, 11))
    assert [tuple(a) for a in o.alleles.tolist()] == alleles and counts.dtype == np.int32 and labels.dtype == np.int32


def test_oracles_agree_on_random_pedigrees():
    rng = np.random.default_rng(1971)
    seen = np.zeros(9, dtype=np.int64)
    for case in range(50):
        ind, fa, mo, pro = random_case(rng, int(rng.integers(5, 201)))
        seed = int(rng.integers(0, 2**63)) * 2 + case % 2
        labels, counts, alleles = ident_literal(ind, fa, mo, pro, 130, seed)
        o = IdentVector(ind, fa, mo, pro)
        assert [tuple(a) for a in o.alleles.tolist()] == alleles, case
        assert np.array_equal(labels, o.labels(130, seed)), case
        assert np.array_equal(counts, o.counts(130, seed)), case
        seen += counts.sum(axis=(0, 1))
    assert np.all(seen > 0)


def test_all_nine_states_occur_on_geneaJi(gen):
    ped = gen.genealogy(gen.geneaJi)
    c = IdentVector(*_args(ped), gen.pro(ped)).counts(5000, 7)
    assert np.all(c.sum(axis=(0, 1)) > 0)


def _check_plan(gen, ind, fa, mo, pro):
    h = gen.IdentityPlan(ind, fa, mo, pro, simul_no=64, seed=1)
    try:
        o = IdentVector(ind, fa, mo, pro)
        assert (h.n_live, h.levels, h.n_labels, h.planes) == (o.n_live, o.levels, o.n_labels, o.planes)
        assert np.array_equal(h.rows_per_level(), o.rows_per_level)
        got = h.alleles()
        assert got.dtype == np.int64 and np.array_equal(got, o.alleles)
        # the live founders and half-founders are the IDs of the table: with n_live and the rows per level they pin the live set
        st = h.stats()
        assert st["sweep_ms"] == 0.0 and st["pair_ms"] == 0.0 and st["planes"] == o.planes and st["levels"] == o.levels
        assert st["tile_rows"] >= 1 and st["tile_cols"] >= 1 and (st["panel_cols"], st["panels"], st["lanes_per_row"]) == (128, 1, 1)
        return o
    finally:
        h.close()


@pytest.mark.parametrize("name", ["geneaJi.csv", "genea140.csv"])
def test_plan_matches_oracle_on_bundled_pedigrees(gen, name):
    ped = gen.genealogy(os.path.join(DATA, name))
    o = _check_plan(gen, *_args(ped), gen.pro(ped))
    assert o.n_labels == 2 * len(np.intersect1d(gen.founder(ped), ped.ind[o.live])) + int(((o.fa < 0) != (o.mo < 0))[o.live].sum())
    _check_plan(gen, *_args(ped), gen.pro(ped)[[2, 0, 2]])
    _check_plan(gen, *_args(ped), ped.ind[:1])                      # a founder alone: 2 labels, one plane, one level
    _check_plan(gen, *_args(ped), ped.ind)


def test_plan_matches_oracle_on_random_pedigrees(gen):
    rng = np.random.default_rng(99)
    live, planes = 0, set()
    for _ in range(200):
        ind, fa, mo, pro = random_case(rng, int(rng.integers(1, 400)))
        o = _check_plan(gen, ind, fa, mo, pro)
        live += o.n_live
        planes.add(o.planes)
    assert live > 1000 and len(planes) >= 4


def test_planned_shapes(gen):
    ind, fa, mo = shapes_pedigree()
    h = gen.IdentityPlan(ind, fa, mo, [8, 6, 8], simul_no=5000, seed=3, panel_cols=1000)
    try:
        assert (h.n_live, h.levels, h.n_labels, h.planes, h.n_pro, h.simul_no, h.seed) == (8, 4, 5, 3, 3, 5000, 3)
        assert h.rows_per_level().tolist() == [2, 2, 3, 1]                           # 1 2 | 3 4 | 5 6 7 | 8: 7 = (0, 4) is on level 2
        assert h.alleles().tolist() == [[1, 0], [1, 1], [2, 0], [2, 1], [7, 0]]
        st = h.stats()
        assert (st["panel_cols"], st["panels"], st["lanes_per_row"]) == (1024, 5, 8)
    finally:
        h.close()
    h = gen.IdentityPlan(ind, fa, mo, [9], simul_no=1, seed=0)
    assert (h.n_live, h.levels, h.n_labels, h.planes) == (1, 1, 2, 1)
    h.close()


def test_argument_errors(gen):
    ind, fa, mo = shapes_pedigree()
    ok = dict(pro_ids=[8, 6], simul_no=10, seed=3)

    def plan(**kw):
        a = {**ok, **kw}
        gen.IdentityPlan(a.pop("ind", ind), a.pop("fa", fa), a.pop("mo", mo), **a).close()

    plan()
    plan(simul_no=1 << 24)
    plan(simul_no=1, labels=True, all_pairs=True, panel_cols=7)
    plan(pro_ids=[8] * 46340)                                                        # 46340^2 < 2^31
    with pytest.raises(KeyError):
        plan(pro_ids=[8, 99])
    with pytest.raises(KeyError):
        plan(pro_ids=[0])
    for kw in (dict(simul_no=0), dict(simul_no=-5), dict(simul_no=(1 << 24) + 1), dict(pro_ids=[]), dict(pro_ids=[8] * 46341), dict(panel_cols=-1)):
        with pytest.raises(ValueError):
            plan(**kw)
    with pytest.raises(Exception, match="duplicate"):
        plan(ind=np.array([1, 2, 3, 4, 5, 6, 7, 8, 1]))
    with pytest.raises(Exception, match="rank order"):
        plan(fa=np.array([8, 0, 1, 1, 3, 3, 0, 5, 0]))
    # the C entry point itself: NULL out, an unknown flag
    L = gen._capi.lib()
    i64 = ctypes.POINTER(ctypes.c_int64)
    pro = np.array([8], dtype=np.int64)
    a = [len(ind), ind.ctypes.data_as(i64), fa.ctypes.data_as(i64), mo.ctypes.data_as(i64), 1, pro.ctypes.data_as(i64), 10, 3, 0]
    h = ctypes.c_void_p()
    assert L.genphi_ident_create(*a, 4, ctypes.byref(h)) == gen._capi.GENPHI_ERR_ARG and not h.value
    assert L.genphi_ident_create(*a, 0, None) == gen._capi.GENPHI_ERR_ARG
    assert L.genphi_ident_levels(None, None, None, None) == gen._capi.GENPHI_ERR_ARG
    assert L.genphi_ident_counts_to_host(None, None) == gen._capi.GENPHI_ERR_ARG
    # nothing computed yet; labels without the flag
    hp = gen.IdentityPlan(ind, fa, mo, [8, 6], simul_no=10, seed=3)
    with pytest.raises(ValueError, match="nothing computed"):
        hp.counts_to_host()
    with pytest.raises(ValueError, match="GENPHI_IDENT_FLAG_LABELS"):
        hp.labels_to_host()
    hp.close()
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(9, dtype=np.int64)}, sort=False)
    with pytest.raises(ValueError):
        gen.simuIdentity(ped, pro=[])
    with pytest.raises(KeyError):
        gen.simuIdentity(ped, pro=[77])
    with pytest.raises(ValueError):
        gen.simuIdentity(ped, simulNo=0)
    with pytest.raises(TypeError):
        gen.simuIdentity(ped, probRecomb=(0.0, 0.0))
    h1, h2 = gen.IdentityPlan(ind, fa, mo, [8]), gen.IdentityPlan(ind, fa, mo, [8])
    assert 0 <= h1.seed < 2**64 and h1.seed != h2.seed and h1.simul_no == 5000
    h1.close()
    h2.close()


def test_symbols_are_exported_declared_and_bound(gen):
    from genlib_jl_amd import _capi
    header = open(os.path.join(ROOT, "include", "genphi.h")).read()
    L = ctypes.CDLL(_capi.LIB_PATH)
    names = ["genphi_ident_" + n for n in ("create", "levels", "alleles", "compute", "counts_to_host", "labels_to_host", "stats", "destroy")]
    for name in names:
        assert hasattr(L, name) and name in _capi.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, header), name
    assert sum(n.startswith("genphi_ident_") for n in _capi.EXPORTED_SYMBOLS) == 8
    assert len(_capi.lib().genphi_ident_create.argtypes) == 11 and len(_capi.lib().genphi_ident_stats.argtypes) == 12
    for macro, value in (("GENPHI_IDENT_FLAG_LABELS", 1), ("GENPHI_IDENT_FLAG_ALL_PAIRS", 2)):
        assert re.search(r"#define %s %d\b" % (macro, value), header) and getattr(_capi, macro) == value
    assert gen.IdentityPlan is _capi.IdentityPlan and gen.simuIdentity.__doc__ and gen.SimuIdentity.__doc__


def test_SimuIdentity_properties(gen):
    """The coefficients from hand-made counts: every one is an integer count divided by S once."""
    counts = np.zeros((2, 2, 9), dtype=np.int32)
    counts[0, 0] = [3, 0, 0, 0, 0, 0, 7, 0, 0]
    counts[1, 1] = [0, 0, 0, 0, 0, 0, 10, 0, 0]
    counts[0, 1] = [1, 0, 2, 0, 1, 1, 1, 3, 1]
    counts[1, 0] = [1, 0, 1, 1, 2, 0, 1, 3, 1]
    r = gen.SimuIdentity(np.array([5, 6]), counts, 10, 1, np.zeros((2, 2), dtype=np.int64), None)
    assert r.delta.shape == (2, 2, 9) and r.delta.dtype == np.float64 and r.delta[0, 1, 7] == 3 / 10
    assert r.kinship.tolist() == [[(12 + 14) / 40, (4 + 8 + 3) / 40], [(4 + 8 + 3) / 40, 20 / 40]]
    assert r.inbreeding.tolist() == [0.3, 0.0] and r.fraternity.tolist() == [[0.7, 0.1], [0.1, 1.0]]
    assert r.ibd[0, 1].tolist() == [0.1, 0.3, 0.1] and r.inbred.tolist() == [[0.3, 0.5], [0.5, 0.0]]
    assert np.array_equal(r.ibd.sum(axis=-1) + r.inbred, np.ones((2, 2)))
    assert r.labels is None and "2 probands" in repr(r)


@pytest.fixture(scope="module")
def mixed():
    """300 individuals with half-founders and selfing; 14 probands, two of them repeats, one a founder."""
    rng = np.random.default_rng(5)
    ind, fa, mo, _ = random_pedigree(rng, 300, p_founder=0.08, p_one_parent=0.1, p_selfing=0.05, max_back=25)
    pro = rng.choice(ind[100:], size=14, replace=False).astype(np.int64)
    pro[9], pro[13], pro[4] = pro[1], pro[1], ind[0]
    o = IdentVector(ind, fa, mo, pro)
    return ind, fa, mo, pro, o, o.labels(5000, 31)


def test_invariants_on_the_reference(gen, mixed):
    ind, fa, mo, pro, o, labels = mixed
    S = 5000
    c = counts_of(labels)
    assert c.dtype == np.int32 and c.shape == (14, 14, 9) and np.all(c.sum(axis=-1) == S) and c.min() >= 0
    assert np.array_equal(swap_roles(c), c)
    same = pro[:, None] == pro[None, :]
    assert same.sum() == 14 + 6 and np.all(c[same][:, [1, 2, 3, 4, 5, 7, 8]] == 0)        # a diagonal pair or repeats: states 1 and 7 only
    assert np.any(c[same][:, 0] > 0) and np.all(c[4, 4] == [0, 0, 0, 0, 0, 0, S, 0, 0])       # an inbred proband; the founder never is
    assert np.all(c.sum(axis=(0, 1)) > 0)                                                   # every state occurs
    # the label rows of S = 64 and 129 are the first columns of those of S = 5000; another seed gives other labels
    assert np.array_equal(o.labels(64, 31), labels[:, :, :64]) and np.array_equal(o.labels(129, 31), labels[:, :, :129])
    assert not np.array_equal(o.labels(129, 32), labels[:, :, :129])
    # a sub-list of probands gives the sub-block (its allele table is another: the counts do not depend on the labels' names)
    sub = np.array([13, 2, 2, 7])
    o2 = IdentVector(ind, fa, mo, pro[sub])
    assert o2.n_labels < o.n_labels and np.array_equal(o2.counts(S, 31), c[np.ix_(sub, sub)])
    # gen.branching(ped, pro=P) first changes nothing
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)
    pruned = gen.branching(ped, pro=pro)
    assert len(pruned) == o.n_live < len(ped)
    o3 = IdentVector(pruned.ind, pruned.father, pruned.mother, pro)
    assert np.array_equal(o3.alleles, o.alleles) and np.array_equal(o3.labels(S, 31), labels)


@pytest.mark.parametrize("state", [2, 1])
def test_cross_check_with_gene_dropping_on_the_references(mixed, state):
    """Founders listed as ancestors of gen.simuSample with state 2 (1) under the same seed: a proband's count in a simulation is the
    number of its two labels that belong to those founders (to their side-0 alleles)."""
    ind, fa, mo, pro, o, labels = mixed
    founders = ind[(fa == 0) & (mo == 0)]
    marked = founders[::2]
    assert len(marked) >= 5
    sample = SimuVector(ind, fa, mo, pro, marked, np.full(len(marked), state)).sample(5000, 31)
    mine = np.isin(o.alleles[:, 0], marked) & ((o.alleles[:, 1] == 0) | (state == 2))
    want = mine[labels].sum(axis=1).astype(np.int8)
    assert np.array_equal(sample, want) and len(np.unique(want)) == 3


def test_kinship_estimate_meets_the_exact_kinship_on_geneaJi(gen):
    """One condition, not a measurement: the per-simulation score of a pair (1, 1/2, 1/4 or 0) lies in [0, 1], so its standard
    deviation is at most 1/2 and 1 / (2 sqrt(S)) bounds that of the mean of S simulations; the margin 5 / sqrt(S) is ten of them, the
    margin of the gene-dropping tests.  Largest deviation found at S = 5000, seed 7: 0.151 / sqrt(S)."""
    ped = gen.genealogy(gen.geneaJi)
    pro, S = gen.pro(ped), 5000
    est = kinship_of(IdentVector(*_args(ped), pro).counts(S, 7), S)
    exact = ExactKinship(*_args(ped)).float64(pro)
    dev = np.abs(est - exact).max() * np.sqrt(S)
    print("geneaJi, S = %d, seed 7: largest |kinship estimate - exact kinship| = %.3f / sqrt(S)" % (S, dev))
    assert dev <= 5.0


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_plan_as_a_stand_alone_program(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "ident_plan_check")
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra", "-pthread"] + flags + [os.path.join(ROOT, "tests", "ident_plan_check.cpp"), os.path.join(CSRC, "ident.cpp"),
                                                                       os.path.join(CSRC, "ancestor_sweep.cpp"), os.path.join(CSRC, "pedigree_index.cpp"), os.path.join(CSRC, "planner.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if san is not None and build.returncode != 0 and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("this toolchain has no -fsanitize=" + san)
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("GENPHI_ENV_HOOKS", None)
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    if san is not None and run.returncode != 0 and not run.stdout and any(
            t in run.stderr for t in ("unexpected memory mapping", "runtime does not come first", "failed to intercept", "ReserveShadowMemoryRange failed")):
        pytest.skip("the sanitizer runtime does not start in this environment: " + run.stderr[:200])
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    m = SUMMARY.search(run.stdout)
    assert m, run.stdout[-1500:]
    pedigrees, rows, labels, half, selfings, repeats, refusals, planes, levels, violations = (int(v) for v in m.groups())
    assert violations == 0 and pedigrees == 3000 and rows > 50_000 and labels > 20_000 and refusals == 900
    assert min(half, selfings, repeats) > 0 and planes >= 8 and levels >= 50
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
