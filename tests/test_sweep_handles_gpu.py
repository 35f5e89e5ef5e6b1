"""The device blocks of the nine sweep handles (csrc/sweep_device.h: every block a handle holds is a DevBuf it registered with its base).
On geneaJi (29 individuals; 130 simulations for gen.simu and gen.simuIdentity), in one process of its own with a budget that keeps
everything: per kind create, compute() twice with every output read after each (this allocates gen.occ's column sums), the outputs equal
and equal to the kind's oracle, close(); what the closed handle returned to the cache is then, byte for byte, what
tests/golden/sweep_handle_bytes.json holds -- recorded with this file from the library of the commit named there, BEFORE the handles
shared an owner: the same blocks of the same sizes, nothing leaked, nothing sized differently -- and release_cached() leaves nothing.
    python tests/test_sweep_handles_gpu.py ROOT_OF_A_BUILT_CHECKOUT COMMIT > tests/golden/sweep_handle_bytes.json
With two devices a handle also computes on device 0, 1 and 0 again: every block it holds moves with it, the results do not change
(gen.simu and gen.simuIdentity are keyed on seed and IDs: bit for bit), and the closed handle leaves its blocks once on either device."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sweep_handle_bytes.json")
S, SEED = 130, 2024


def kinds(gen):
    """{kind: (make() -> handle, read(handle) -> {output: array}, the oracle's {output: array})} on geneaJi."""
    from completeness_oracle import completeness_exact
    from depths_oracle import depths_exact
    from gc_oracle import gc_literal
    from ident_oracle import IdentVector, counts_of
    from implex_oracle import implex_literal, ind_matrix
    from mrca_oracle import meioses_literal
    from occ_oracle import occ_literal, rec_literal
    from simu_oracle import match_counts, simu_literal, state_counts
    ped = gen.genealogy(gen.geneaJi)
    args = (ped.ind, ped.father, ped.mother)
    pro, fnd = gen.pro(ped), gen.founder(ped)
    states = np.arange(len(fnd)) % 3
    state_pro = np.arange(len(pro)) % 3
    occ = occ_literal(*args, pro, fnd).T
    d = depths_exact(*args, pro, fnd)
    comp_counts, comp_matrix = completeness_exact(*args, pro)
    implex_counts = implex_literal(*args, pro)[0]
    sample = simu_literal(*args, pro, fnd, states, S, SEED)
    labels = IdentVector(*args, pro).labels(S, SEED)
    return {
        "GCPlan": (lambda: gen.GCPlan(*args, pro, fnd), lambda h: {"result": h.result_to_host()}, {"result": gc_literal(*args, pro, fnd)}),
        "OccPlan": (lambda: gen.OccPlan(*args, pro, fnd), lambda h: {"result": h.result_to_host(), "totals": h.totals()},
                    {"result": occ, "totals": occ.sum(axis=0)}),
        "RecPlan": (lambda: gen.RecPlan(*args, pro, fnd), lambda h: {"result": h.result()}, {"result": rec_literal(*args, pro, fnd)}),
        "DistPlan": (lambda: gen.DistPlan(*args, pro, fnd), lambda h: {"result": h.result_to_host()}, {"result": meioses_literal(*args, pro, fnd)}),
        "DepthPlan": (lambda: gen.DepthPlan(*args, pro, fnd), lambda h: dict(zip(("min", "max", "paths", "mean"), h.result_to_host())),
                      {"min": d.min, "max": d.max, "paths": d.paths, "mean": d.mean}),
        "CompletenessPlan": (lambda: gen.CompletenessPlan(*args, pro), lambda h: {"counts": h.counts(), "result": h.result_to_host(), "totals": h.totals()},
                             {"counts": comp_counts, "result": np.ascontiguousarray(comp_matrix.T), "totals": comp_counts.sum(axis=0)}),
        "ImplexPlan": (lambda: gen.ImplexPlan(*args, pro), lambda h: {"counts": h.counts(), "result": h.result_to_host(), "totals": h.totals()},
                       {"counts": implex_counts, "result": np.ascontiguousarray(ind_matrix(implex_counts).T), "totals": implex_counts.sum(axis=0)}),
        "SimuPlan": (lambda: gen.SimuPlan(*args, pro, fnd, states, simul_no=S, seed=SEED),
                     lambda h: {"sample": h.sample_to_host(), "state_counts": h.state_counts(), "match_counts": h.match_counts(state_pro)},
                     {"sample": sample, "state_counts": state_counts(sample), "match_counts": match_counts(sample, state_pro)}),
        "IdentityPlan": (lambda: gen.IdentityPlan(*args, pro, simul_no=S, seed=SEED, labels=True),
                         lambda h: {"counts": h.counts_to_host(), "labels": h.labels_to_host()}, {"counts": counts_of(labels), "labels": labels}),
    }


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].dtype, want[k].shape)
        assert np.array_equal(got[k], want[k], equal_nan=got[k].dtype.kind == "f"), (what, k)


def closed_handle_bytes(root, devices):
    """{kind: cached_bytes() after close()} with the library of the checkout at root; the handle computes on every device of `devices` in turn."""
    sys.path[:0] = [root, HERE]
    import genlib_jl_amd as gen
    from genlib_jl_amd import _capi
    assert os.path.dirname(os.path.dirname(os.path.abspath(_capi.__file__))) == os.path.abspath(root)
    kept = {}
    _capi.release_cached()
    assert _capi.cached_bytes() == 0
    for kind, (make, read, want) in kinds(gen).items():
        h = make()
        for dev in devices:
            h.compute(device=dev)
            _same(read(h), want, (kind, dev))
        h.close()
        kept[kind] = _capi.cached_bytes()
        assert kept[kind] > 0, kind
        _capi.release_cached()
        assert _capi.cached_bytes() == 0, kind
    return kept


def _worker(devices):
    env = dict(os.environ, GENPHI_KEEP_MB="4096", GENPHI_ENV_HOOKS="1")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), os.path.dirname(HERE), "-", ",".join(str(d) for d in devices)],
                         capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    return json.loads(run.stdout)["bytes"]


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["bytes"]


def test_a_closed_handle_returns_the_blocks_of_the_recorded_commit():
    kept, want = _worker([0, 0]), _golden()
    print("bytes a closed handle returns to the cache:", kept)
    assert kept == want


def test_a_handle_moves_between_devices_with_all_its_blocks():
    import ctypes
    n = ctypes.c_int(0)
    assert ctypes.CDLL("libamdhip64.so").hipGetDeviceCount(ctypes.byref(n)) == 0       # (what torch.cuda.device_count() asks, without the import)
    if n.value < 2:
        pytest.skip("one device")
    # computed on 0, moved to 1, moved back to 0 (into the blocks it left there): closed, it leaves one set of blocks on either device
    kept, want = _worker([0, 1, 0]), _golden()
    print("bytes a closed handle returns to the cache after computing on devices 0, 1, 0:", kept)
    assert kept == {kind: 2 * b for kind, b in want.items()}


if __name__ == "__main__":
    root, commit, devices = sys.argv[1], sys.argv[2], [int(d) for d in (sys.argv[3] if len(sys.argv) > 3 else "0,0").split(",")]
    json.dump({"recorded_at_commit": commit, "bytes": closed_handle_bytes(root, devices)}, sys.stdout, indent=1)
    print()
