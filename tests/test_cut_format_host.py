"""The storage format of the early dense cuts (csrc/cut_format.h) without a GPU: tests/cut_format_check.cpp holds the format rule to
its table -- (cut, kind of the step that writes it, format that step reads, kind of the step that reads it) -> Float32 / 16 / 24 bits,
both boundaries (cuts 7 | 8 and 11 | 12), every kind of step that keeps Float32 --, round-trips every 16-bit value and the 24-bit
corners through the very functions the kernels call to encode, pack, unpack and decode a quad of entries, fires their guard on values
that are no integer of the unit, past the range, negative, NaN or infinite, checks the GENPHI_NO_NARROW hook, and holds the narrow forms
of the certified-rows kernel to what they add to the row geometry's invariants.  Built with g++,
once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer (the stand-alone program only)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMARY = re.compile(r"^cut format check: (\d+) checks; (\d+) violations$", re.M)
NO_RUNTIME = ("unexpected memory mapping", "runtime does not come first", "failed to intercept", "ReserveShadowMemoryRange failed")


def _build(gxx, san, exe):
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra", "-pthread"] + flags + [os.path.join(ROOT, "tests", "cut_format_check.cpp"), "-o", exe]
    return subprocess.run(cmd, capture_output=True, text=True)


def _run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)


def _check(run):
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    m = SUMMARY.search(run.stdout)
    assert m, run.stdout[-1500:]
    checks, violations = int(m.group(1)), int(m.group(2))
    assert violations == 0
    assert checks >= 1_000_000           # (the program ran whole: 8 cuts x 65,536 values x 2 alone)
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_cut_format_rule_codec_and_narrow_forms(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "cut_format_check")
    build = _build(gxx, san, exe)
    if san is not None and build.returncode != 0 and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("this toolchain has no -fsanitize=" + san)
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    run = _run(exe)
    if san is not None and run.returncode != 0 and not run.stdout and "VIOLATION" not in run.stderr and any(t in run.stderr for t in NO_RUNTIME):
        # the sanitizer's runtime did not start: no finding about the code only if the same source passes without it
        plain = str(tmp_path / "cut_format_check_plain")
        assert _build(gxx, None, plain).returncode == 0
        _check(_run(plain))
        pytest.skip("the sanitizer runtime does not start in this environment: " + run.stderr[:200])
    _check(run)
