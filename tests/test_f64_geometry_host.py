"""The launch geometry of the Float64-storage level kernels (csrc/f64_geometry.h) without a GPU: tests/f64_geometry_check.cpp walks every
source cut of 0 .. 21,000 members with the plan's row pitch for that size and with pitches up to 45,056, for 1, 7 and 100,000 rows, 1 and
256 CUs, both kernel settings and the LDS budgets 160 KB, 4 x 300, 4 x 2048 and 4 x 8192 bytes, and holds each geometry to its invariants:
the form is the one the budget allows (full up to 10,239 members, split up to 20,479, per-entry beyond, at the default budget), the
per-thread staging pieces cover the source row and the per-thread columns the output row, source indices fit the 16 bits they are packed
into, the LDS request is within the budget and the grid within 1 .. rows.  Built with g++, once plain and once under AddressSanitizer +
UndefinedBehaviorSanitizer (the stand-alone program only)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SUMMARY = re.compile(r"^f64 geometry check: (\d+) checks, (\d+) full, (\d+) split and (\d+) naive launches; (\d+) violations$", re.M)
NO_RUNTIME = ("unexpected memory mapping", "runtime does not come first", "failed to intercept", "ReserveShadowMemoryRange failed")


def _build(gxx, san, exe):
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra"] + flags + [os.path.join(ROOT, "tests", "f64_geometry_check.cpp"), "-o", exe]
    return subprocess.run(cmd, capture_output=True, text=True)


def _run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)


def _check(run):
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    m = SUMMARY.search(run.stdout)
    assert m, run.stdout[-1500:]
    checks, full, split, naive, violations = (int(v) for v in m.groups())
    assert violations == 0
    # the program ran whole: 21,001 cuts x 14 pitches x 49 launches, and every form was met many times over
    assert full + split + naive == 21001 * 14 * 49 and checks >= 50_000_000
    assert min(full, split, naive) >= 1_000_000
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_f64_geometry_invariants(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "f64_geometry_check")
    build = _build(gxx, san, exe)
    if san is not None and build.returncode != 0 and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("this toolchain has no -fsanitize=" + san)
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    run = _run(exe)
    if san is not None and run.returncode != 0 and not run.stdout and "VIOLATION" not in run.stderr and any(t in run.stderr for t in NO_RUNTIME):
        # The sanitizer's runtime did not start: the program printed nothing.  That is no finding about the code only if the same source
        # passes without it, so the plain build is made and run here before the skip is allowed.
        plain = str(tmp_path / "f64_geometry_check_plain")
        assert _build(gxx, None, plain).returncode == 0
        _check(_run(plain))
        pytest.skip("the sanitizer runtime does not start in this environment: " + run.stderr[:200])
    _check(run)
