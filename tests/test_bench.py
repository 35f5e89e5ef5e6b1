"""bench.py's own contract.  A plain run measures the headline only: --steps timed sweeps, `ms_per_step` on the line, and with
--dump-outputs the matrix the last timed sweep computed -- what gen.phi hands its caller -- written for comparison between
builds.  --full adds the measurements that take runs of their own (hipGraph replay, device-to-host copy, CPU baseline, call walls)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_dump_outputs_refuses_paths_without_a_resident_matrix(tmp_path):
    for extra in (["--dry-run"], ["--workload", "sparse140"], ["--exchange"]):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", str(tmp_path)] + extra, cwd=ROOT,
                             capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and "--dump-outputs" in out.stderr, out.stderr[-2000:]
    assert not os.listdir(tmp_path)


@pytest.mark.gpu
def test_plain_run_dumps_what_the_last_step_computed(tmp_path):
    d = _bench("--workload", "cfg2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "proband-pairs/s" and d["higher_is_better"] is True
    assert "cpu_baseline" not in d and "other_workloads" not in d                       # (--full only)
    assert "d2h_ms" not in d["end_to_end"] and "call_wall" not in d["end_to_end"] and d["roofline"]["graph_replay_ms_per_step"] is None
    gold = np.load(os.path.join(HERE, "golden", "genea140_phi_oracle.npy"))         # 140 x 140: small enough to be dumped whole
    rows, diag = np.load(tmp_path / "phi_rows.npy"), np.load(tmp_path / "phi_diag.npy")
    assert rows.dtype == diag.dtype == np.float32
    assert np.array_equal(rows, gold) and np.array_equal(diag, np.diag(gold))


@pytest.mark.gpu
def test_full_run_adds_the_measurements_of_their_own():
    d = _bench("--workload", "cfg2", "--steps", "2", "--warmup", "1", "--full")
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    assert d["roofline"]["graph_replay_ms_per_step"] > 0 and d["end_to_end"]["d2h_ms"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["end_to_end"]["call_wall"]["first_ms"] > 0
