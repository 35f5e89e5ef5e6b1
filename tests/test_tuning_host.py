"""The hooks of a plan (csrc/tuning.h) without a GPU.  tests/tuning_check.cpp holds tuning_from to literal expectations: the defaults, every
hook at a value of its own, the quirks of the parsing (presence hooks are set by "0", GENPHI_STAY_TILE takes 128 or 256 only, a malformed
GENPHI_SHARD_FORCE is ignored, GENPHI_NEAREST_BUF is clamped and rounded ...), and what plan_options_from / sparse_tuning_from hand on.  Built with
g++, once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer (the stand-alone program only).  Through the C ABI, with no
device: genphi_tuning_set accepts the 50 names it always did, and README.md's table of hooks and that list cover each other."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SUMMARY = re.compile(r"^tuning check: (\d+) checks; (\d+) violations$", re.M)
NO_RUNTIME = ("unexpected memory mapping", "runtime does not come first", "failed to intercept", "ReserveShadowMemoryRange failed")

# the names genphi_tuning_set accepted before the table of csrc/tuning.h replaced the hand-kept list
NAMES = """LDS_CAP_FLOATS FULL_MAX_FLOATS NO_STAY STAY_MAX_SLOTS STAY_HEADROOM STAY_MEM_PCT STAY_SCATTER STAY_TWO_PASS STAY_COL_FASTEST STAY_SCALAR_T
STAY_TILE STAY_SLACK_PCT STAY_MIN_RATIO_PCT STAY_NARROW STAY_NARROW_MIN STAY_OVERHEAD_K STAY_LAST COLPERM_PLAIN STAY_FAMILY MAX_GROUP MAX_RUN FULL_BS
NO_IDENTITY CERT_MIN_EXP DBG_STEP NO_FAST MAX_CPT FAST_NT WIDE_ROUTE TT_NOALIGN NO_SHARD_PRUNE SHARD_FORCE SHARD_PRUNE_MIN_STEP NO_SMALL NO_GRAPH
D2H_THREADS D2H_PAGEABLE D2H_SYM D2H_TILE D2H_CHUNK_MB TEST_FAIL_ALLOC SPARSE_K SPARSE_PERMILLE SPARSE_MIN_CUT SPARSE_CHUNK SPARSE_CLASSES SPARSE_BATCH
SPARSE_ARENA BOOT_PANEL NEAREST_BUF""".split()

# GENPHI_ names of README.md's "Environment hooks" that are no settings of a plan: the gate and the ungated variables, hooks that other
# handles read for themselves, the Python mirror's and bench.py's, and a build macro
NOT_PLAN_HOOKS = {"GENPHI_ENV_HOOKS", "GENPHI_TRACE", "GENPHI_KEEP_MB", "GENPHI_SPARSE_KEEP_MB", "GENPHI_PLAN_CACHE", "GENPHI_FORCE_EXCHANGE", "GENPHI_PLAN_THREADS",
                  "GENPHI_D2H_STATS", "GENPHI_PANEL_NAIVE", "GENPHI_SPARSE_NO_FUSED", "GENPHI_SPARSE_STALE_CAP", "GENPHI_WG_TIMES",
                  "GENPHI_OCC_PANEL", "GENPHI_OCC_PANELS_PER_LAUNCH", "GENPHI_OCC_ROWS", "GENPHI_OCC_ROWS64", "GENPHI_DIST_PANEL", "GENPHI_DIST_PANELS_PER_LAUNCH",
                  "GENPHI_IMPLEX_PANEL", "GENPHI_IMPLEX_PANELS_PER_LAUNCH", "GENPHI_SIMU_PANEL", "GENPHI_GC_PANEL", "GENPHI_GC_PANELS_PER_LAUNCH"}


def _build(gxx, san, exe):
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra"] + flags + [os.path.join(ROOT, "tests", "tuning_check.cpp"), "-o", exe]
    return subprocess.run(cmd, capture_output=True, text=True)


def _run(exe):
    # (the program sets the variables it reads itself: none of the session's hooks may reach it)
    env = {k: v for k, v in os.environ.items() if not k.startswith("GENPHI_")}
    env.update(ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)


def _check(run):
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    m = SUMMARY.search(run.stdout)
    assert m, run.stdout[-1500:]
    checks, violations = (int(v) for v in m.groups())
    assert violations == 0
    assert checks >= 400                                   # (the program ran whole: six comparisons of 52 fields and the names)
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_tuning_from_against_literal_expectations(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "tuning_check")
    build = _build(gxx, san, exe)
    if san is not None and build.returncode != 0 and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("this toolchain has no -fsanitize=" + san)
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    run = _run(exe)
    if san is not None and run.returncode != 0 and not run.stdout and "VIOLATION" not in run.stderr and any(t in run.stderr for t in NO_RUNTIME):
        # The sanitizer's runtime did not start: the program printed nothing.  That is no finding about the code only if the same source
        # passes without it, so the plain build is made and run here before the skip is allowed.
        plain = str(tmp_path / "tuning_check_plain")
        assert _build(gxx, None, plain).returncode == 0
        _check(_run(plain))
        pytest.skip("the sanitizer runtime does not start in this environment: " + run.stderr[:200])
    _check(run)


def _accepts(L, t, name):
    return L.genphi_tuning_set(t, name.encode(), b"1")


def test_tuning_set_accepts_the_names_it_always_did(gen):
    L = gen._capi.lib()
    assert len(NAMES) == 50 and len(set(NAMES)) == 50
    t = L.genphi_tuning_create()
    try:
        for name in NAMES:
            assert _accepts(L, t, name) == 0, name
            assert _accepts(L, t, "GENPHI_" + name) == 0, name
        assert _accepts(L, t, "GENPHI_NOPE") != 0
        assert gen._capi.last_error() == "genphi_tuning_set: unknown setting GENPHI_NOPE"
        assert _accepts(L, t, "NOPE") != 0
        assert gen._capi.last_error() == "genphi_tuning_set: unknown setting GENPHI_NOPE"
    finally:
        L.genphi_tuning_destroy(t)


def test_readme_lists_the_hooks_and_only_them(gen):
    text = open(os.path.join(ROOT, "README.md")).read()
    begin = text.index("Tuning hooks of `libgenphi.so`")
    table = text.index("| variable | effect |", begin)
    rows = re.match(r"(?:\|.*\n?)+", text[table:]).group(0)             # the table's lines: up to the first line that is no row
    section = text[begin:table] + rows
    listed = set(re.findall(r"GENPHI_[A-Z0-9_]+", section))
    assert len(listed) > 60                                 # (the section was found whole)
    L = gen._capi.lib()
    t = L.genphi_tuning_create()
    try:
        for name in NAMES:
            assert "GENPHI_" + name in listed, name
        for name in sorted(listed - NOT_PLAN_HOOKS):
            assert _accepts(L, t, name) == 0, name + " is in README.md but is no setting of a plan"
        for name in sorted(NOT_PLAN_HOOKS):
            assert name in listed and _accepts(L, t, name) != 0, name
    finally:
        L.genphi_tuning_destroy(t)
