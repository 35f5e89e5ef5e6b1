"""DevBuf (csrc/devbuf.h), the owner of every cached device block of a plan, without a GPU: tests/devbuf_check.cpp gives it a cache made
of host malloc with a table of live blocks and a switch that fails the k-th allocation, and checks that reserve grows and never shrinks,
that the recorded count is the request (0 included), that a failed reserve leaves no pointer and no capacity behind (so a later, smaller
request allocates again), that release is idempotent, that moves empty their source and free the destination's old block once, and that
nothing is live or freed twice at the end.  Built with g++ -- the header needs hipError_t from <hip/hip_runtime_api.h>, no HIP language --
once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer (the stand-alone program only)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genlib.jl_amd", "csrc")

SUMMARY = re.compile(r"^devbuf check: (\d+) checks, (\d+) allocations, (\d+) frees, (\d+) bad frees, (\d+) live blocks; (\d+) violations$", re.M)
NO_RUNTIME = ("unexpected memory mapping", "runtime does not come first", "failed to intercept", "ReserveShadowMemoryRange failed")


def _hip_include():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")                      # (where build() looks for the compiler)
    return os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")


def _build(gxx, san, exe):
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-isystem", _hip_include()] + flags + [os.path.join(ROOT, "tests", "devbuf_check.cpp"), "-o", exe]
    return subprocess.run(cmd, capture_output=True, text=True)


def _run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)


def _check(run):
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    m = SUMMARY.search(run.stdout)
    assert m, run.stdout[-1500:]
    checks, allocs, frees, bad_frees, live, violations = (int(v) for v in m.groups())
    assert violations == 0 and bad_frees == 0 and live == 0
    assert checks >= 40 and allocs == frees and allocs >= 15       # (the program ran whole)
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_devbuf_against_a_host_cache(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "devbuf_check")
    build = _build(gxx, san, exe)
    if san is not None and build.returncode != 0 and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("this toolchain has no -fsanitize=" + san)
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    run = _run(exe)
    if san is not None and run.returncode != 0 and not run.stdout and "VIOLATION" not in run.stderr and any(t in run.stderr for t in NO_RUNTIME):
        # The sanitizer's runtime did not start: the program printed nothing.  That is no finding about the code only if the same source
        # passes without it, so the plain build is made and run here before the skip is allowed.
        plain = str(tmp_path / "devbuf_check_plain")
        assert _build(gxx, None, plain).returncode == 0
        _check(_run(plain))
        pytest.skip("the sanitizer runtime does not start in this environment: " + run.stderr[:200])
    _check(run)


def test_the_owner_has_no_hip_language_in_it():
    """devbuf.h, device_sizes.h, tuning.h and row_geometry.h stay host only: that is what lets the stand-alone checkers build them with g++."""
    host_only = ("#include <hip", "__global__", '#include "resident.h"', '#include "sparse_levels.h"', '#include "panel_launch.h"')
    for name, banned in (("devbuf.h", ("<hip/hip_runtime.h>", '#include "devcache.h"', "__global__")), ("device_sizes.h", ("#include <hip", '#include "dev')),
                         ("tuning.h", host_only), ("row_geometry.h", host_only)):
        text = open(os.path.join(CSRC, name)).read()
        assert not any(b in text for b in banned), name
