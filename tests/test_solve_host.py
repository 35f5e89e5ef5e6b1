"""The conjugate-gradient core of genphi_result_solve (csrc/result_solve.cpp: genphi::cg_solve) without a GPU: tests/solve_check.cpp
hands it a host product over dense Float64 matrices of known spectrum and checks the iteration that include/genphi.h states --
residuals and iteration counts against their derived bounds, a column alone against the column in company bit for bit, a singular and a
negative definite matrix, a right-hand side in the null space, a zero column, NaN and inf in b and in the matrix, max_iter = 1, a
failing product, pitches beyond k.  Built with g++ from the checker and result_solve.cpp -- no HIP -- once plain and once under
AddressSanitizer + UndefinedBehaviorSanitizer (the stand-alone program only)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genlib.jl_amd", "csrc")

SUMMARY = re.compile(r"^solve check: (\d+) systems, (\d+) columns, (\d+) products; (\d+) violations$", re.M)
NO_RUNTIME = ("unexpected memory mapping", "runtime does not come first", "failed to intercept", "ReserveShadowMemoryRange failed")


def _build(gxx, san, exe):
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra"] + flags + [os.path.join(ROOT, "tests", "solve_check.cpp"), os.path.join(CSRC, "result_solve.cpp"), "-o", exe]
    return subprocess.run(cmd, capture_output=True, text=True)


def _run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)


def _check(run):
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    m = SUMMARY.search(run.stdout)
    assert m, run.stdout[-1500:]
    systems, columns, products, violations = (int(v) for v in m.groups())
    assert violations == 0
    assert systems >= 400 and columns >= 1000 and products > systems
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_conjugate_gradients_over_a_host_product(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "solve_check")
    build = _build(gxx, san, exe)
    if san is not None and build.returncode != 0 and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("this toolchain has no -fsanitize=" + san)
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    run = _run(exe)
    if san is not None and run.returncode != 0 and not run.stdout and "VIOLATION" not in run.stderr and any(t in run.stderr for t in NO_RUNTIME):
        # The sanitizer's runtime did not start: the program printed nothing, not even its first check.  That is no finding about the
        # code only if the same sources pass without it, so the plain build is made and run here before the skip is allowed.
        plain = str(tmp_path / "solve_check_plain")
        assert _build(gxx, None, plain).returncode == 0
        _check(_run(plain))
        pytest.skip("the sanitizer runtime does not start in this environment: " + run.stderr[:200])
    _check(run)


def test_the_core_has_no_hip_in_it():
    """result_solve.h / .cpp stay host only: that is what lets this file build them without a GPU toolchain."""
    for name in ("result_solve.h", "result_solve.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "resident.h" not in text, name
