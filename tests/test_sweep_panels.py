"""The column panels of the ancestor sweeps (csrc/sweep_panels.h: plan_panels), without a GPU: tests/sweep_panels_check.cpp compares every
layout with the arithmetic of gen.gc, gen.occ, gen.rec and gen.meioses written out one sweep at a time, with layouts derived by hand, and
with what a layout has to satisfy (pitch, panels per launch, device room, coverage of the columns).  Built with g++ from the checker and
the header -- no HIP -- once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SUMMARY = re.compile(r"^sweep panels: (\d+) layouts against the sweeps' own formulas \((\d+) fit, (\d+) do not\), (\d+) by hand; (\d+) violations$", re.M)


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_panel_layouts(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "sweep_panels_check")
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra"] + flags + [os.path.join(ROOT, "tests", "sweep_panels_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if san is not None and build.returncode != 0 and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("this toolchain has no -fsanitize=" + san)
    assert build.returncode == 0, build.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    if san is not None and run.returncode != 0 and not run.stdout and any(
            t in run.stderr for t in ("unexpected memory mapping", "runtime does not come first", "failed to intercept", "ReserveShadowMemoryRange failed")):
        pytest.skip("the sanitizer runtime does not start in this environment: " + run.stderr[:200])
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    m = SUMMARY.search(run.stdout)
    assert m, run.stdout[-1500:]
    layouts, fit, no_fit, by_hand, violations = (int(v) for v in m.groups())
    assert violations == 0
    # 5 rules (both occ widths) x 6 slot counts x 15 column counts x 8 panel hooks x 3 per-launch hooks x 4 device rooms
    assert layouts == 5 * 6 * 15 * 8 * 3 * 4 and fit + no_fit == layouts and min(fit, no_fit) > 0 and by_hand == 9
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
