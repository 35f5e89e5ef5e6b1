"""Host side of gen.phiHist / gen.phiQuantile (no GPU): the two forms of the oracle of tests/phi_hist_oracle.py against each other,
the numpy forms of the package on host matrices against them, the exported symbols, the argument checks genphi_result_hist and
genphi_result_select make on a plan that has never computed, and the host arithmetic of csrc/hist_geometry.h
(tests/hist_geometry_check.cpp, built with g++ plainly and under AddressSanitizer + UndefinedBehaviorSanitizer)."""
import ctypes
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import phi_hist_oracle as HO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_pinned.json")))
GOLDEN140 = os.path.join(ROOT, "tests", "golden", "genea140_phi_oracle.npy")
POP140 = os.path.join(ROOT, "tests", "golden", "pop140.csv")


def _ji():
    return np.array(GOLD["geneaJi"]["phi"], dtype=np.float32)


def _random37():
    """A symmetric 37 x 37 Float32 matrix with planted ties and zeros."""
    rng = np.random.default_rng(37)
    a = rng.random((37, 37)).astype(np.float32) * np.float32(0.5)
    a[rng.random((37, 37)) < 0.3] = 0.0                                     # zeros
    a[rng.random((37, 37)) < 0.2] = np.float32(0.125)                        # ties
    a[rng.random((37, 37)) < 0.1] = np.float32(0.25)
    m = np.maximum(a, a.T)
    np.fill_diagonal(m, 0.5)
    return m


EDGE_SETS = [np.linspace(0.0, 0.5, 9), np.array([0.0, 0.125, 0.25, 0.5]), np.array([0.125, 0.25]), np.array([-math.inf, 0.0, 1e-30, 0.125, math.inf]),
             np.array([0.3, 0.4]), np.array([0.0, float(np.nextafter(np.float64(0.125), 1.0)), 0.25])]


@pytest.mark.parametrize("matrix", ["geneaJi", "random37"])
def test_the_two_oracle_forms_and_the_package_agree(gen, matrix):
    m = _ji() if matrix == "geneaJi" else _random37()
    n = len(m)
    labels = (np.arange(n) % 3).astype(np.int32)
    labels[::5] = -1                                                        # an unlabelled proband in every pattern
    if n == 3:
        labels = np.array([0, 1, 0], dtype=np.int32)
    ids = 100 + 3 * np.arange(n)
    groups = {int(i): "g%d" % g for i, g in zip(ids, labels) if g >= 0}
    g = int(labels.max()) + 1
    for edges in EDGE_SETS + [np.array([float(m[0, 1]), float(m[0, 2]) if m[0, 2] > m[0, 1] else float(m[0, 1]) + 0.01])]:
        ref = HO.hist_loop(m, edges)
        assert HO.same(HO.hist(m, edges), ref)
        assert HO.total(*ref) == n * (n - 1) // 2
        got = gen.phiHist(m, bins=edges)
        assert HO.same((got.counts, got.below, got.above), ref) and got.n_pairs == n * (n - 1) // 2 and got.names is None
        assert np.array_equal(got.edges, edges) and got.counts.dtype == np.int64
        refg = HO.hist_loop(m, edges, labels, g)
        assert HO.same(HO.hist(m, edges, labels, g), refg)
        assert np.array_equal(refg[0], np.transpose(refg[0], (1, 0, 2))) and np.array_equal(refg[1], refg[1].T)
        lab_only = np.nonzero(labels >= 0)[0]
        sub = HO.hist_loop(m[np.ix_(lab_only, lab_only)], edges)
        upper = np.triu(np.ones((g, g), dtype=bool))
        assert np.array_equal(refg[0][upper].sum(axis=0), sub[0]) and refg[1][upper].sum() == sub[1] and refg[2][upper].sum() == sub[2]
        got = gen.phiHist(m, bins=edges, groups=groups, probandIDs=ids)
        assert got.names == sorted(set(groups.values())) and HO.same((got.counts, got.below, got.above), refg)
        assert got.sizes.tolist() == np.bincount(labels[labels >= 0], minlength=g).tolist() and got.n_pairs == HO.total(*refg)
    # shards add; the last row has no pair
    parts = [HO.hist(m[a:b], EDGE_SETS[0], labels, g, row_begin=a) for a, b in ((0, 1), (1, n - 1), (n - 1, n))]
    assert HO.same(tuple(sum(p[k] for p in parts) for k in range(3)), HO.hist(m, EDGE_SETS[0], labels, g))
    assert HO.total(*HO.hist(m[n - 1:], EDGE_SETS[0], row_begin=n - 1)) == 0 and HO.n_pairs(n, 0, n) == n * (n - 1) // 2


def test_an_edge_on_a_data_value_and_the_closed_last_bin(gen):
    m = np.array([[.5, .25, .125, 0], [.25, .5, 0, .125], [.125, 0, .5, .0625], [0, .125, .0625, .5]], dtype=np.float32)
    got = gen.phiHist(m, bins=[0.0, 0.125, 0.25])                           # pairs: .25 .125 0 0 .125 .0625
    assert got.counts.tolist() == [3, 3] and got.below == 0 and got.above == 0 and got.n_pairs == 6      # .125 opens bin 1; .25 closes it
    got = gen.phiHist(m, bins=[0.0625, 0.125])
    assert got.counts.tolist() == [3] and got.below == 2 and got.above == 1
    got = gen.phiHist(m, bins=[float(np.nextafter(np.float64(0.0625), 1.0)), 0.2])
    assert got.counts.tolist() == [2] and got.below == 3 and got.above == 1
    got = gen.phiHist(m, bins=2, range=(0.0, 0.25))
    assert got.edges.tolist() == [0.0, 0.125, 0.25] and got.counts.tolist() == [3, 3]
    got = gen.phiHist(m)                                                    # 64 bins over [0, 0.5]
    assert len(got.counts) == 64 and got.counts.sum() == 6 and got.counts[0] == 2 and "6 pairs" in repr(got)
    assert np.array_equal(got.counts, np.histogram(m[np.triu_indices(4, 1)].astype(np.float64), bins=64, range=(0.0, 0.5))[0])
    g = gen.phiHist(m, bins=[0.0, 0.125, 0.25], groups={1: "a", 2: "a", 3: "b"}, probandIDs=[1, 2, 3, 4])
    assert g.names == ["a", "b"] and g.sizes.tolist() == [2, 1] and g.n_pairs == 3 and "2 groups" in repr(g)
    assert g.counts.tolist() == [[[0, 1], [1, 1]], [[1, 1], [0, 0]]]


def test_phiQuantile_of_a_host_matrix_is_numpys_linear_method(gen):
    for m in (_ji(), _random37(), np.load(GOLDEN140)):
        x = m[np.triu_indices(len(m), 1)].astype(np.float64)
        q = np.array([0.0, 0.01, 0.25, 0.5, 1 / 3, 0.75, 0.9, 0.99, 0.999, 1.0, 0.5])
        got = gen.phiQuantile(m, q)
        ref = np.quantile(x, q, method="linear")
        assert got.dtype == np.float64 and got.shape == q.shape
        assert np.all(np.abs(got - ref) <= 1e-15 * np.abs(ref)), (got, ref)
        assert np.array_equal(got, HO.quantile(m, q))
        assert gen.phiQuantile(m, 0.5).shape == (1,) and gen.phiQuantile(m, 1.0)[0] == x.max() and gen.phiQuantile(m, 0.0)[0] == x.min()
    assert np.array_equal(HO.select(_random37(), [0, 665, 5, 5]), np.sort(_random37()[np.triu_indices(37, 1)])[[0, 665, 5, 5]])


def test_argument_errors_of_the_package(gen):
    m = _random37()
    for bad in ([0.0], [0.0, 0.0], [0.1, 0.0], [0.0, math.nan], np.zeros((2, 2)), np.arange(4098.0)):
        with pytest.raises(ValueError):
            gen.phiHist(m, bins=bad)
    for bad in (0, -3):
        with pytest.raises(ValueError):
            gen.phiHist(m, bins=bad)
    with pytest.raises(ValueError):
        gen.phiHist(m, bins=4, range=(0.5, 0.0))
    with pytest.raises(ValueError):
        gen.phiHist(m[:3])
    with pytest.raises(ValueError):
        gen.phiHist(m, groups={1: "a"})                                     # groups of a host matrix need the IDs of its rows
    with pytest.raises(ValueError):
        gen.phiHist(m, groups={}, probandIDs=np.arange(37))
    with pytest.raises(ValueError):
        gen.phiHist(m, bins=4096, groups={k: k % 5 for k in range(37)}, probandIDs=np.arange(37))      # 5 x 4096 cells
    for bad in (-0.1, 1.5, math.nan, [[0.5]]):
        with pytest.raises(ValueError):
            gen.phiQuantile(m, bad)
    with pytest.raises(ValueError):
        gen.phiQuantile(m[:1, :1], 0.5)                                     # one proband: no pair
    ped = gen.genealogy(gen.geneaJi)
    with pytest.raises(KeyError):
        gen.phiHist(ped, probandIDs=[1, 12345])
    with pytest.raises(KeyError):
        gen.phiQuantile(ped, 0.5, probandIDs=[1, 12345])
    with pytest.raises(ValueError):
        gen.phiHist(ped, bins=[0.1, 0.1])
    with pytest.raises(ValueError):
        gen.phiQuantile(ped, 2.0)


def test_symbols_are_exported_declared_and_bound(gen):
    from genlib_jl_amd import _capi
    header = open(os.path.join(ROOT, "include", "genphi.h")).read()
    for name, n_args in (("genphi_result_hist", 9), ("genphi_result_select", 5)):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(_capi.LIB_PATH), name)
        assert re.search(r"\b%s\s*\(" % name, header) and len(getattr(_capi.lib(), name).argtypes) == n_args
    for macro, value in (("GENPHI_HIST_MAX_EDGES", 4097), ("GENPHI_HIST_MAX_GROUPS", 256), ("GENPHI_HIST_MAX_CELLS", 16384), ("GENPHI_SELECT_MAX_RANKS", 16)):
        assert re.search(r"#define %s %d\b" % (macro, value), header) and getattr(_capi, macro) == value
    for name in ("phiHist", "phiQuantile", "PhiHist"):
        assert hasattr(gen, name)
    for name in ("hist", "select", "count_pairs"):
        assert hasattr(gen.PhiPlan, name)


def test_argument_errors_on_a_plan_that_has_never_computed(gen):
    ped = gen.genealogy(gen.genea140)
    pl = gen.plan(ped)
    L, C = gen._capi.lib(), gen._capi
    n = pl.n_probands
    assert n == 140
    dp, i32p, i64p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    npairs = ctypes.c_int64(-7)

    def hist(edges, labels=None, g=0, n_edges=None):
        e = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32)
        return L.genphi_result_hist(pl._h, (len(e) if n_edges is None else n_edges), None if e is None else e.ctypes.data_as(dp), g,
                                    None if lab is None else lab.ctypes.data_as(i32p), None, None, None, ctypes.byref(npairs))

    def select(ranks, n_ranks=None, values=True):
        r = None if ranks is None else np.ascontiguousarray(ranks, dtype=np.int64)
        v = np.zeros(32, dtype=np.float32)
        return L.genphi_result_select(pl._h, (len(r) if n_ranks is None else n_ranks), None if r is None else r.ctypes.data_as(i64p),
                                      v.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if values else None, ctypes.byref(npairs))

    ok = np.zeros(n, dtype=np.int32)
    try:
        for call, text in ((lambda: hist(None, n_edges=3), "edges is NULL"), (lambda: hist([0.0]), "n_edges = 1"), (lambda: hist(np.arange(4098.0)), "n_edges = 4098"),
                         (lambda: hist([0.0, 0.2, 0.2]), "strictly increasing"), (lambda: hist([0.0, 0.3, 0.2]), "strictly increasing"),
                         (lambda: hist([0.0, math.nan, 0.2]), "NaN"), (lambda: hist([math.nan, 0.2]), "NaN"),
                         (lambda: hist(np.arange(4097.0), ok, 5), "cells"), (lambda: hist(np.arange(66.0), ok, 256), "cells"),
                         (lambda: hist([0.0, 0.5], np.where(np.arange(n) == 7, -2, 0), 2), "label -2"), (lambda: hist([0.0, 0.5], np.where(np.arange(n) == 7, 2, 0), 2), "label 2"),
                         (lambda: hist([0.0, 0.5], ok, 0), "n_groups"), (lambda: hist([0.0, 0.5], ok, 257), "n_groups"), (lambda: hist([0.0, 0.5], None, 2), "n_groups"),
                         (lambda: select(np.zeros(17), 17), "n_ranks = 17"), (lambda: select(np.zeros(1), -1), "n_ranks = -1"), (lambda: select(None, 1), "ranks is NULL"),
                         (lambda: select(np.zeros(1), 1, values=False), "values is NULL"), (lambda: select(None, 0, values=True), "n_ranks = 0")):
            rc = call()
            assert rc == C.GENPHI_ERR_ARG and text in C.last_error(), (rc, text, C.last_error())
        assert L.genphi_result_hist(None, 2, np.zeros(2).ctypes.data_as(dp), 0, None, None, None, None, None) == C.GENPHI_ERR_ARG
        assert L.genphi_result_select(None, 0, None, None, None) == C.GENPHI_ERR_ARG
        assert npairs.value == -7                                            # no output is written after an error
        # valid arguments: only the resident result is missing
        for call in (lambda: hist([0.0, 0.5]), lambda: hist(np.arange(4097.0)), lambda: hist(np.arange(65.0), ok, 256), lambda: hist([-math.inf, 0.0, math.inf], ok - 1, 1), lambda: select([0]),
                   lambda: select(np.arange(16)), lambda: select(None, 0, values=False)):
            rc = call()
            assert rc == C.GENPHI_ERR_DEVICE and "no resident result" in C.last_error()
        assert npairs.value == -7                                            # ... nor after this one
        for call in (lambda: pl.hist([0.0, 0.5]), lambda: pl.hist([0.0, 0.5], ok), lambda: pl.select([0]), lambda: pl.count_pairs()):
            with pytest.raises(gen.GenphiDeviceError):
                call()
        for call in (lambda: pl.hist([0.0]), lambda: pl.hist([0.5, 0.0]), lambda: pl.hist([0.0, math.nan]), lambda: pl.hist([0.0, 0.5], ok[:5]),
                     lambda: pl.hist([0.0, 0.5], ok, 257), lambda: pl.hist(np.arange(4097.0), ok, 5), lambda: pl.hist([0.0, 0.5], ok + 3, 2),
                     lambda: pl.hist([0.0, 0.5], None, 3), lambda: pl.select([[0]])):
            with pytest.raises(ValueError):
                call()
    finally:
        pl.close()
    pl = gen.plan(gen.genealogy(gen.geneaJi), [29])                         # N < 2: no pair exists, with or without a result
    try:
        c, b, a = pl.hist([0.0, 0.5])
        assert c.tolist() == [0] and b == 0 and a == 0 and pl.count_pairs() == 0
        c, b, a = pl.hist([0.0, 0.25, 0.5], [0], 1)
        assert c.shape == (1, 1, 2) and not c.any() and not b.any() and not a.any()
        c, b, a = pl.hist([0.0, 0.25, 0.5], [-1])                           # nobody labelled, n_groups left out: one empty group
        assert c.shape == (1, 1, 2) and not c.any() and b.shape == (1, 1)
        with pytest.raises(ValueError):
            pl.select([0])                                                  # no pair: every rank is out of range
    finally:
        pl.close()


# ---- csrc/hist_geometry.h ---------------------------------------------------------------------------------------------------------

SUMMARY = re.compile(r"^hist geometry check: (\d+) checks, (\d+) walks, (\d+) edges; (\d+) violations$", re.M)
NO_RUNTIME = ("unexpected memory mapping", "runtime does not come first", "failed to intercept", "ReserveShadowMemoryRange failed")


def _build(gxx, san, exe):
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra"] + flags + [os.path.join(ROOT, "tests", "hist_geometry_check.cpp"), "-o", exe]
    return subprocess.run(cmd, capture_output=True, text=True)


def _run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)


def _check(run):
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    m = SUMMARY.search(run.stdout)
    assert m, run.stdout[-1500:]
    checks, walks, edges, violations = (int(v) for v in m.groups())
    assert violations == 0 and walks >= 300 and edges >= 10_000 and checks >= 1_000_000
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_hist_geometry_invariants(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "hist_geometry_check")
    build = _build(gxx, san, exe)
    if san is not None and build.returncode != 0 and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("this toolchain has no -fsanitize=" + san)
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    run = _run(exe)
    if san is not None and run.returncode != 0 and not run.stdout and "VIOLATION" not in run.stderr and any(t in run.stderr for t in NO_RUNTIME):
        # The sanitizer's runtime did not start: the program printed nothing.  That is no finding about the code only if the same source
        # passes without it, so the plain build is made and run here before the skip is allowed.
        plain = str(tmp_path / "hist_geometry_check_plain")
        assert _build(gxx, None, plain).returncode == 0
        _check(_run(plain))
        pytest.skip("the sanitizer runtime does not start in this environment: " + run.stderr[:200])
    _check(run)
