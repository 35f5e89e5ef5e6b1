"""PhiPlan.device_bytes_needed (host only: genphi_plan_device_bytes_needed, whose level-buffer, parent-matrix, result and final_tmp terms
come from csrc/device_sizes.h -- the function the allocations themselves use) equals, with ==, what tests/golden/device_bytes_needed.json
records for a fixed list of plans.  The file was recorded from the build before device_sizes.h existed, when the estimate carried its own
copy of every formula.  `python tests/test_device_sizes_host.py --record` rewrites it (no GPU needed)."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "device_bytes_needed.json")
HOOKS = ("GENPHI_LDS_CAP_FLOATS", "GENPHI_SPARSE_K", "GENPHI_STAY_LAST", "GENPHI_STAY_MEM_PCT", "GENPHI_STAY_NARROW_MIN", "GENPHI_STAY_OVERHEAD_K")


def _cases():
    """(name, pedigree, environment hooks): the pedigrees of test_sweep_host_contract.py under its hooks, geneaJi, genea140."""
    stay = {"GENPHI_LDS_CAP_FLOATS": "256", "GENPHI_STAY_MEM_PCT": "100000", "GENPHI_STAY_NARROW_MIN": "0", "GENPHI_STAY_OVERHEAD_K": "0"}
    out = [("geneaJi", "geneaJi", {}), ("genea140 pro", "genea140", {}), ("genea140 quarter", "genea140 quarter", {})]
    out += [(f"mating cap={cap}", "mating", {} if cap is None else {"GENPHI_LDS_CAP_FLOATS": str(cap)}) for cap in (None, 2048, 1500, 300)]
    out += [("deep", "deep", {}), ("founders", "founders", {})]
    out += [(f"stay last={last}", "stay", dict(stay, GENPHI_STAY_LAST=last)) for last in ("1", "0")]
    out += [("mating sparse_k=-1", "mating", {"GENPHI_SPARSE_K": "-1"}), ("genea140 pro sparse_k=-1", "genea140", {"GENPHI_SPARSE_K": "-1"})]
    return out


def _pedigree(gen, name):
    if name.startswith("genea"):
        ped = gen.genealogy(getattr(gen, name.split()[0]))
        if name.endswith("quarter"):         # (the proband set of test_plan_memory_estimate_and_kept_blocks: the proband cut stays in place)
            return ped, np.sort(np.random.default_rng(7).choice(np.asarray(ped.ind), size=len(ped.ind) // 4, replace=False))
        return ped, gen.pro(ped)
    from test_sweep_host_contract import _ped
    ind, fa, mo, sex, pro = _ped(name)
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}), pro


def _needed(gen, peds, ped_name, env):
    saved = {k: os.environ.pop(k, None) for k in HOOKS}
    os.environ.update(env)
    try:
        if ped_name not in peds:
            peds[ped_name] = _pedigree(gen, ped_name)
        pl = gen.plan(*peds[ped_name])
        need = pl.device_bytes_needed
        assert pl.device_bytes == 0          # (asking uploads nothing)
        pl.close()
        return need
    finally:
        for k in HOOKS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def _run_all(gen):
    peds = {}
    return {name: _needed(gen, peds, ped, env) for name, ped, env in _cases()}


def test_device_bytes_needed_is_what_it_was(gen):
    want = json.load(open(GOLDEN))
    got = _run_all(gen)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_device_sizes_host.py --record    (from the build to pin)"
    os.environ["GENPHI_ENV_HOOKS"] = "1"
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import genlib_jl_amd
    with open(GOLDEN, "w") as f:
        json.dump(_run_all(genlib_jl_amd), f, indent=0, sort_keys=True)
        f.write("\n")
