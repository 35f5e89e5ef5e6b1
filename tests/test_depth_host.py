"""gen.depths on the CPU: the word arithmetic of csrc/depth_word.h on the host schedule (tests/depth_check.cpp, plain and under
AddressSanitizer + UndefinedBehaviorSanitizer), the two oracles of tests/depths_oracle.py against each other and against closed forms,
the refusals of genphi_depth_create (no device is needed to plan), and the exports."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import depths_oracle as DO
from random_pedigree import random_pedigree
from test_occ_reference import doubling_chain, quirk_pedigree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genlib.jl_amd", "csrc")

SUMMARY = re.compile(r"^depth check: (\d+) pedigrees, (\d+) schedules, (\d+) rows \((\d+) copy items\), (\d+) entries compared; (\d+) one-parent members, "
                     r"(\d+) probands with children, (\d+) probands that are listed ancestors, (\d+) lists with duplicated probands, "
                     r"(\d+) with duplicated ancestors, (\d+) pairs without a path; largest P (\d+), longest ascent (\d+); (\d+) ladders of 47 steps; "
                     r"(\d+) violations$", re.M)


def _args(ped):
    return ped.ind, ped.father, ped.mother


def skipping_ladder():
    """doubling_chain(48) whose last member has a mate from generation 46 instead of 47: min 46 < mean < max 47 to either founder."""
    ind, fa, mo = doubling_chain(48)
    mo = mo.copy()
    mo[95] = 92                                   # ID 96 = (93, 92): 92 is a member of generation 46
    return ind, fa, mo


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_depth_words_on_random_schedules_and_the_ladders(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "depth_check")
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra", "-pthread"] + flags + [os.path.join(ROOT, "tests", "depth_check.cpp"),
                                                                       os.path.join(CSRC, "ancestor_sweep.cpp"), os.path.join(CSRC, "planner.cpp"), "-o", exe]
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
    (pedigrees, schedules, rows, copies, entries, one_parent, with_children, pro_is_anc, dup_pro, dup_anc, unrelated, max_paths, longest, ladders,
     violations) = (int(v) for v in m.groups())
    assert violations == 0
    assert pedigrees >= 2000 and schedules >= 2 * pedigrees and rows > 20_000 and entries > 100_000
    assert min(copies, one_parent, with_children, pro_is_anc, dup_pro, dup_anc, unrelated) > 0           # every edge was reached
    assert ladders == 2 and max_paths == 2 ** 46 and longest == 47                                       # the packed fields at their limit
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]


def _same(a, b):
    for name in ("min", "max", "paths"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(a.mean, b.mean, equal_nan=True)
    assert a.P == b.P and a.S == b.S


def test_the_two_oracles_agree(gen):
    ped = gen.genealogy(gen.geneaJi)
    everyone = ped.ind
    _same(DO.depths_literal(*_args(ped), everyone, everyone), DO.depths_exact(*_args(ped), everyone, everyone))
    d = DO.depths_exact(*_args(ped), gen.pro(ped), gen.founder(ped))
    assert d.paths.shape == (3, 6) and int(d.paths.sum()) > 18 and d.min.min() >= -1
    for by in ("proband", "ancestor"):
        _same(DO.reduce_depths(DO.depths_literal(*_args(ped), [1, 2, 29, 2], [17, 19, 20, 14]), by),
              DO.reduce_depths(DO.depths_exact(*_args(ped), [1, 2, 29, 2], [17, 19, 20, 14]), by))
    rng = np.random.default_rng(20261019)
    for case in range(40):
        n = int(rng.integers(1, 40))
        ind, fa, mo, _ = random_pedigree(rng, n, p_founder=0.15, p_one_parent=0.2, p_selfing=0.05, max_back=int(rng.integers(2, 12)), max_depth=9)
        pro = rng.integers(1, n + 1, size=int(rng.integers(0, 8)))
        anc = rng.integers(1, n + 1, size=int(rng.integers(0, 12)))
        lit, exact = DO.depths_literal(ind, fa, mo, pro, anc), DO.depths_exact(ind, fa, mo, pro, anc)
        _same(lit, exact)
        for by in ("proband", "ancestor"):
            _same(DO.reduce_depths(lit, by), DO.reduce_depths(exact, by))


def test_oracle_on_a_hand_made_pedigree(gen):
    """quirk_pedigree (tests/test_occ_reference.py): 12 = (8, 9) reaches 1 by 1-3-6-8-12, 1-3-7-8-12, 1-4-7-8-12 (4 meioses) and 1-4-9-12 (3)."""
    ped = quirk_pedigree(gen)
    for fn in (DO.depths_literal, DO.depths_exact):
        d = fn(*_args(ped), [12, 8, 10, 12], [1, 8, 11, 1, 10])
        assert d.paths.tolist() == [[4, 1, 0, 4, 0], [3, 1, 0, 3, 0], [0, 0, 0, 0, 1], [4, 1, 0, 4, 0]]
        assert d.min.tolist() == [[3, 1, -1, 3, -1], [3, 0, -1, 3, -1], [-1, -1, -1, -1, 0], [3, 1, -1, 3, -1]]
        assert d.max.tolist() == [[4, 1, -1, 4, -1], [3, 0, -1, 3, -1], [-1, -1, -1, -1, 0], [4, 1, -1, 4, -1]]
        assert d.mean[0, 0] == 15 / 4 and d.mean[1, 1] == 0.0 and np.isnan(d.mean[0, 2]) and d.mean[2, 4] == 0.0
        r = DO.reduce_depths(fn(*_args(ped), [12, 8, 10, 12], [1, 8, 11, 10]), "proband")
        assert (r.paths.tolist(), r.min.tolist(), r.max.tolist()) == ([5, 4, 1, 5], [1, 0, 0, 1], [4, 3, 0, 4]) and r.mean[0] == 16 / 5
        r = DO.reduce_depths(fn(*_args(ped), [12, 8, 10, 12], [1, 8, 11, 1]), "ancestor")
        assert (r.paths.tolist(), r.min.tolist(), r.max.tolist()) == ([11, 3, 0, 11], [3, 0, -1, 3], [4, 1, -1, 4]) and np.isnan(r.mean[2])
        assert r.mean[0] == 39 / 11
        with pytest.raises(KeyError):
            fn(*_args(ped), [8, 99], [1])
        with pytest.raises(KeyError):
            fn(*_args(ped), [8], [99])


def test_exact_oracle_on_the_ladders_and_genea140(gen):
    """The sib-mating ladder of tests/depth_check.cpp through the other oracle: 2^46 paths of 47 meioses per founder; with one
    generation-skipping mate 2^45 of 47 and 2^44 of 46.  genea140: the figures the bound of 47 steps is far from."""
    d = DO.depths_exact(*doubling_chain(48), [96, 95], [1, 2])
    assert d.paths.tolist() == [[2 ** 46] * 2] * 2 and d.S[0][0] == 47 * 2 ** 46 and d.min.tolist() == d.max.tolist() == [[47, 47]] * 2
    assert d.mean.tolist() == [[47.0, 47.0]] * 2
    d = DO.depths_exact(*skipping_ladder(), [96, 95], [1, 2])
    assert d.paths[0].tolist() == [3 * 2 ** 44] * 2 and d.S[0][1] == 47 * 2 ** 45 + 46 * 2 ** 44
    assert d.min[0].tolist() == [46, 46] and d.max[0].tolist() == [47, 47] and d.mean[0, 0] == 140 / 3
    assert d.paths[1].tolist() == [2 ** 46] * 2
    ped = gen.genealogy(gen.genea140)
    d = DO.depths_exact(*_args(ped), gen.pro(ped), gen.founder(ped))
    assert d.paths.shape == (140, 7399)
    assert (int(d.max.max()), int(d.paths.max()), max(max(row) for row in d.S)) == (17, 176, 2313)


def _ladder_plan(gen, times, by):
    ind, fa, mo = doubling_chain(48)
    return gen.DepthPlan(ind, fa, mo, [96] * times, [1, 2], by=by)


def test_create_refusals_need_no_device(gen):
    from genlib_jl_amd import _capi
    assert _capi.GENPHI_DEPTH_MAX_STEPS == 47
    header = open(os.path.join(ROOT, "include", "genphi.h")).read()
    assert "#define GENPHI_DEPTH_MAX_STEPS 47" in header
    for k, name in enumerate(("PAIR", "PROBAND", "ANCESTOR")):
        assert "#define GENPHI_DEPTH_BY_%s %d" % (name, k) in header and _capi.GENPHI_DEPTH_BY[name.lower()] == k
    # 47 steps plan, 48 are refused
    ind, fa, mo = doubling_chain(48)
    for by in ("pair", "proband"):
        gen.DepthPlan(ind, fa, mo, [96, 95], [1, 2], by=by).close()
    ind, fa, mo = doubling_chain(49)
    for by in ("pair", "proband", "ancestor"):
        with pytest.raises(ValueError, match="48 steps.*at most 47"):
            gen.DepthPlan(ind, fa, mo, [98], [1], by=by)
    gen.DepthPlan(ind, fa, mo, [96, 3], [1]).close()                 # the limit is about the listed probands
    # by = proband adds over the columns: no ancestor twice; the other modes take duplicates
    ped = quirk_pedigree(gen)
    with pytest.raises(ValueError, match="twice"):
        gen.DepthPlan(*_args(ped), [12, 8], [1, 3, 1], by="proband")
    for by in ("pair", "ancestor"):
        gen.DepthPlan(*_args(ped), [12, 8], [1, 3, 1], by=by).close()
    gen.DepthPlan(*_args(ped), [12, 12], [1, 3], by="proband").close()
    # by = ancestor: n_pro * steps * 2^steps < 2^63.  2048 * 47 * 2^47 = 2^63.55, 1024 * 47 * 2^47 = 2^62.55
    with pytest.raises(ValueError, match="Int64"):
        _ladder_plan(gen, 2048, "ancestor")
    h = _ladder_plan(gen, 1024, "ancestor")
    assert h.shape == (2,)
    h.close()
    for by in ("pair", "proband"):
        _ladder_plan(gen, 2048, by).close()
    # an unknown by, negative panel arguments
    for by in (3, -1, "founder"):
        with pytest.raises(ValueError):
            gen.DepthPlan(*_args(ped), [12], [1], by=by)
    with pytest.raises(ValueError):
        gen.depths(ped, by="both")
    for kw in ({"panel_cols": -1}, {"panels_per_launch": -2}):
        with pytest.raises(ValueError):
            gen.DepthPlan(*_args(ped), [12], [1], **kw)
    # unknown IDs
    with pytest.raises(KeyError):
        gen.DepthPlan(*_args(ped), [8, 99], [1])
    with pytest.raises(KeyError):
        gen.DepthPlan(*_args(ped), [8], [1, 99])
    with pytest.raises(KeyError):
        gen.depths(ped, pro=[0])
    with pytest.raises(KeyError):
        gen.genMean(ped, [99])


def test_plans_shapes_and_empty_results_without_a_device(gen):
    ped = quirk_pedigree(gen)
    for by, shape in (("pair", (4, 3)), ("proband", (4,)), ("ancestor", (3,))):
        h = gen.DepthPlan(*_args(ped), [12, 8, 3, 12], [1, 5, 11], by=by, panel_cols=2, panels_per_launch=1)
        try:
            assert h.shape == shape
            st = h.stats()
            assert st["peak_slots"] > 0 and st["sweep_ms"] == 0.0 and st["launches"] == 0
        finally:
            h.close()
    # nothing to compute: no device is needed
    for pro, anc in (([], [1, 2]), ([8, 9], []), ([], [])):
        for by, shape in (("pair", (len(pro), len(anc))), ("proband", (len(pro),)), ("ancestor", (len(anc),))):
            d = gen.depths(ped, pro=pro, ancestors=anc, by=by)
            assert d.by == by and d.pro.tolist() == pro and d.ancestors.tolist() == anc
            assert d.min.shape == d.max.shape == d.mean.shape == d.paths.shape == shape
            assert (d.min.dtype, d.max.dtype, d.mean.dtype, d.paths.dtype) == (np.int16, np.int16, np.float64, np.int64)
            assert (d.min == -1).all() and (d.max == -1).all() and (d.paths == 0).all() and np.isnan(d.mean).all()
    assert gen.genMin(ped, []).shape == (0,) and gen.genMax(ped, []).dtype == np.int16 and gen.genMean(ped, []).dtype == np.float64


def test_symbols_are_exported_and_called_by_the_julia_shim(gen):
    from genlib_jl_amd import _capi
    src = open(os.path.join(ROOT, "genlib.jl_amd", "julia", "GenLibAMD.jl")).read()
    called = set(re.findall(r"\(:(genphi_depth_[a-z_]+), libgenphi\)", src))
    assert called == {"genphi_depth_create", "genphi_depth_compute", "genphi_depth_shape", "genphi_depth_result_to_host", "genphi_depth_destroy"}
    header = open(os.path.join(ROOT, "include", "genphi.h")).read()
    L = ctypes.CDLL(_capi.LIB_PATH)
    for name in called | {"genphi_depth_result_device", "genphi_depth_stats"}:
        assert hasattr(L, name) and name in _capi.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, header), name
    assert sum(name.startswith("genphi_depth_") for name in _capi.EXPORTED_SYMBOLS) == 7
    assert gen.DepthPlan is _capi.DepthPlan
    for fn in (gen.depths, gen.genMin, gen.genMax, gen.genMean):
        assert fn.__doc__
    for name in ("min", "max", "mean"):                            # the builtins the module uses stay what they are
        assert not hasattr(gen, name)
    # the create call of the shim passes the three Int32 arguments of the header, in its order
    assert re.search(r"Int64, Ptr\{Int64\}, Int64, Ptr\{Int64\}, Int32, Int32, Int32, Ptr\{Ptr\{Cvoid\}\}\),\s*length\(ind\), ind, father, mother, "
                     r"length\(pro\), pro, length\(ancestors\), ancestors, DEPTH_BY\[by\], Int32\(0\), Int32\(0\), h\)", src)
    assert re.search(r"int32_t by,\s*int32_t panel_cols, int32_t panels_per_launch, genphi_depth \*\*out\)", header)
