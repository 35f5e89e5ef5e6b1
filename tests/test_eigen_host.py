"""The Lanczos core of genphi_result_eigen (csrc/result_eigen.cpp: genphi::lanczos_top, genphi::tridiagonal_ql) without a GPU:
tests/eigen_check.cpp hands it host callbacks over dense Float64 matrices of known spectrum (a diagonal under a Householder similarity,
N = 1 .. 200) and checks the iteration that include/genphi.h states -- values against the spectrum within the reported residual, the
residual against a recomputed one, the flags against the residuals, unit norm, orthogonality and the sign rule, k = N, a multiple top
eigenvalue, I / 2 (a breakdown at every step), a start vector inside a small invariant subspace, max_iter = k, tol = 0, centring
against a Jacobi solver, NaN and inf in the matrix, every callback failing, and the tridiagonal solver against a dense Jacobi on the
same T.  Built with g++ from the checker and result_eigen.cpp -- no HIP -- once plain and once under AddressSanitizer +
UndefinedBehaviorSanitizer (the stand-alone program only)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genlib.jl_amd", "csrc")

SUMMARY = re.compile(r"^eigen check: (\d+) matrices, (\d+) pairs, (\d+) products; (\d+) violations$", re.M)
NO_RUNTIME = ("unexpected memory mapping", "runtime does not come first", "failed to intercept", "ReserveShadowMemoryRange failed")


def _build(gxx, san, exe):
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra"] + flags + [os.path.join(ROOT, "tests", "eigen_check.cpp"), os.path.join(CSRC, "result_eigen.cpp"), "-o", exe]
    return subprocess.run(cmd, capture_output=True, text=True)


def _run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)


def _check(run):
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    m = SUMMARY.search(run.stdout)
    assert m, run.stdout[-1500:]
    matrices, pairs, products, violations = (int(v) for v in m.groups())
    assert violations == 0
    assert matrices >= 150 and pairs >= 150 and products > pairs
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_lanczos_over_host_callbacks(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "eigen_check")
    build = _build(gxx, san, exe)
    if san is not None and build.returncode != 0 and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("this toolchain has no -fsanitize=" + san)
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    run = _run(exe)
    if san is not None and run.returncode != 0 and not run.stdout and "VIOLATION" not in run.stderr and any(t in run.stderr for t in NO_RUNTIME):
        # The sanitizer's runtime did not start: the program printed nothing, not even its first check.  That is no finding about the
        # code only if the same sources pass without it, so the plain build is made and run here before the skip is allowed.
        plain = str(tmp_path / "eigen_check_plain")
        assert _build(gxx, None, plain).returncode == 0
        _check(_run(plain))
        pytest.skip("the sanitizer runtime does not start in this environment: " + run.stderr[:200])
    _check(run)


def test_the_core_has_no_hip_in_it():
    """result_eigen.h / .cpp stay host only: that is what lets this file build them without a GPU toolchain."""
    for name in ("result_eigen.h", "result_eigen.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "resident.h" not in text, name
