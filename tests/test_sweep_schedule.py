"""The host schedule that gen.gc, gen.occ, gen.rec, gen.meioses and gen.completeness share (csrc/ancestor_sweep.cpp: plan_sweep) on
random pedigrees, without a GPU: tests/sweep_schedule_check.cpp checks every schedule as a structure (which rows exist, which slot
each lives in, when a slot is handed out again, copy items, one-hot columns, peak_slots), interprets its items on the CPU in the
arithmetic of each caller and compares every result row with a top-down recursion over the pedigree.  Built with g++ from the checker,
ancestor_sweep.cpp and planner.cpp -- no HIP, no oracle -- once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genlib.jl_amd", "csrc")

SUMMARY = re.compile(r"^sweep schedules: (\d+) checked \((\d+) by hand\), (\d+) lists, (\d+) items \((\d+) copy items\), (\d+) result entries compared; "
                     r"(\d+) of one cut, (\d+) without probands, (\d+) with an unknown ID refused, (\d+) with unknown probands dropped, "
                     r"(\d+) slots handed out again; (\d+) violations$", re.M)


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_sweep_schedules_of_random_pedigrees(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "sweep_schedule_check")
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra", "-pthread"] + flags + [os.path.join(ROOT, "tests", "sweep_schedule_check.cpp"),
                                                                       os.path.join(CSRC, "ancestor_sweep.cpp"), os.path.join(CSRC, "planner.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if san is not None and build.returncode != 0 and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("this toolchain has no -fsanitize=" + san)
    assert build.returncode == 0, build.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("GENPHI_ENV_HOOKS", None)
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    if san is not None and run.returncode != 0 and not run.stdout and any(
            t in run.stderr for t in ("unexpected memory mapping", "runtime does not come first", "failed to intercept", "ReserveShadowMemoryRange failed")):
        pytest.skip("the sanitizer runtime does not start in this environment: " + run.stderr[:200])
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    m = SUMMARY.search(run.stdout)
    assert m, run.stdout[-1500:]
    schedules, by_hand, lists, items, copies, entries, one_cut, no_pro, refused, dropped, reused, violations = (int(v) for v in m.groups())
    assert violations == 0
    assert schedules >= 5000 and by_hand == 45 and lists > schedules and items > 100_000 and entries > 1_000_000
    assert min(copies, one_cut, no_pro, refused, dropped, reused) > 0          # every edge was reached, and slots were reused
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
