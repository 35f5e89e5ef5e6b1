"""The pedigree index that the host plans of gen.simu, gen.simuIdentity and gen.implex share (csrc/pedigree_index.cpp) and the
rows-by-level builder and panel width of the two gene-dropping plans (csrc/drop_plan.h), as a stand-alone program
(tests/pedigree_index_check.cpp): random pedigrees of 1-200 individuals with IDs on both sides of the switch between the direct table
and the hash map, checked against a brute-force restatement; the empty pedigree, nobody live, a single level.  Built with g++ from the
checker and pedigree_index.cpp -- no HIP -- once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genlib.jl_amd", "csrc")
SUMMARY = re.compile(r"pedigree_index_check: (\d+) pedigrees, (\d+) rows, (\d+) direct tables, (\d+) hash maps, (\d+) refusals, (\d+) with nobody live, "
                     r"(\d+) of one level, (\d+) violations")


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_index_and_rows_as_a_stand_alone_program(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "pedigree_index_check")
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra"] + flags + [os.path.join(ROOT, "tests", "pedigree_index_check.cpp"),
                                                             os.path.join(CSRC, "pedigree_index.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if san is not None and build.returncode != 0 and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("this toolchain has no -fsanitize=" + san)
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    if san is not None and run.returncode != 0 and not run.stdout and any(
            t in run.stderr for t in ("unexpected memory mapping", "runtime does not come first", "failed to intercept", "ReserveShadowMemoryRange failed")):
        pytest.skip("the sanitizer runtime does not start in this environment: " + run.stderr[:200])
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    m = SUMMARY.search(run.stdout)
    assert m, run.stdout[-1500:]
    pedigrees, rows, direct, hashed, refusals, nobody, one_level, violations = (int(v) for v in m.groups())
    assert violations == 0 and pedigrees == 400 and direct == 200 and hashed == 200 and rows > 10_000
    assert refusals >= 75 and nobody >= 15 and one_level >= 30
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
