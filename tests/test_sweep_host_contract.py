"""The host side of a Float32 sweep, held to what it did before it was split into phases: for a fixed list of small plans and call
sequences, the outcome of every call (error class and text, stats.n_steps, every stats.level_rows[s] -- the observable of the shard
pruning --, the plan's device bytes after the call, a SHA-256 of the host copy of the result) equals, with ==, what
tests/golden/sweep_host_contract.json records.  `python tests/test_sweep_host_contract.py --record` rewrites that file on a GPU."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sweep_host_contract.json")
HOOKS = ("GENPHI_LDS_CAP_FLOATS", "GENPHI_NO_SHARD_PRUNE", "GENPHI_NO_SMALL", "GENPHI_STAY_LAST", "GENPHI_STAY_MEM_PCT", "GENPHI_STAY_NARROW_MIN",
         "GENPHI_STAY_OVERHEAD_K", "GENPHI_TEST_FAIL_ALLOC")


def _ped(name):
    from genlib_jl_amd import synth
    if name == "mating":
        return synth.random_mating(8000, 900, 9, skip_permille=40)
    if name == "deep_shallow":           # a deep family and an unrelated shallow one: upper levels with no rows for a shard of the latter
        deep, shallow = synth.deep_inbred(60, 30, 3), synth.deep_inbred(12, 24, 2, seed=5)
        n1 = len(deep[0])
        rel = lambda a: np.where(a > 0, a + n1, 0)                           # noqa: E731
        return (np.concatenate([deep[0], shallow[0] + n1]), np.concatenate([deep[1], rel(shallow[1])]),
                np.concatenate([deep[2], rel(shallow[2])]), np.concatenate([deep[3], shallow[3]]), np.concatenate([deep[4], shallow[4] + n1]))
    if name == "deep":                   # 39 level steps: the third call with the same arguments replays a captured graph
        return synth.deep_inbred(40, 40, 3)
    if name == "stay":                   # overlapping generations, every individual a proband: the proband cut may stay in place (Plan::final_slots)
        ind, fa, mo, sex, _ = synth.random_mating(500, 30, 5, skip_permille=400, seed=1)
        return ind, fa, mo, sex, ind.copy()
    if name == "founders":               # every proband parentless: no level step
        ind, fa, mo, sex, _ = synth.random_mating(300, 40, 4, seed=3)
        return ind, fa, mo, sex, np.asarray([i for i, f, m in zip(ind, fa, mo) if f == 0 and m == 0][:7])
    if name == "upload":
        return synth.random_mating(3000, 300, 8, skip_permille=100)
    raise KeyError(name)


def _call(rows=None, **kw):
    return dict(rows=rows, **kw)


def _cases():
    """(name, pedigree, environment hooks, calls).  A negative row counts from the number of probands."""
    shards = [(0, 1), (1, 130), (130, 131), (131, 600), (600, -1), None, (5, 17)]
    out = []
    for cap in (None, 2048, 1500, 300):  # last step FULL (2048: under SPLIT upper steps), SPLIT (a WIDE step among the upper ones), WIDE
        for prune in (True, False):
            env = {} if cap is None else {"GENPHI_LDS_CAP_FLOATS": str(cap)}
            if not prune:
                env["GENPHI_NO_SHARD_PRUNE"] = "1"
            calls = [_call(r) for r in shards] + [_call((131, 600), timing=True), _call((1, 130), kernel=1), _call(None, kernel=1),
                                                 _call((130, 131), kernel=1, timing=True), _call((1, 130))]
            out.append((f"mating cap={cap} prune={int(prune)}", "mating", env, calls))
    k, n = 30, 54                        # (probands of the deep family, of both)
    for small_off in (False, True):
        calls = [_call(None), _call((k, n)), _call((0, k)), _call((k - 3, k + 5)), _call((k, n), kernel=1), _call((k, n), timing=True)]
        out.append((f"deep_shallow no_small={int(small_off)}", "deep_shallow", {"GENPHI_NO_SMALL": "1"} if small_off else {}, calls))
    A, B = (3, 11), (0, 40)
    out.append(("deep graph A A B A A", "deep", {}, [_call(A), _call(A), _call(A), _call(B), _call(A), _call(A), _call(A), _call(None),
                                                     _call(A, timing=True), _call(A, kernel=1), _call(A, kernel=1), _call(A, kernel=1)]))
    for last in ("1", "0"):
        env = {"GENPHI_LDS_CAP_FLOATS": "256", "GENPHI_STAY_MEM_PCT": "100000", "GENPHI_STAY_NARROW_MIN": "0", "GENPHI_STAY_OVERHEAD_K": "0",
               "GENPHI_STAY_LAST": last}
        out.append((f"stay last={last}", "stay", env, [_call(None), _call((5, 100)), _call((5, 100)), _call((0, 5), timing=True),
                                                        _call((100, -1), kernel=1), _call(None)]))
    out.append(("founders only", "founders", {}, [_call(None), _call((2, 5)), _call(None, timing=True), _call((0, 1), kernel=1)]))
    out.append(("empty shard after Float64", "mating", {}, [_call((3, 40), storage64=True), _call((7, 7)), _call((3, 40)), _call((900, 900))]))
    for k in range(1, 13):               # (one small upload makes fewer allocations than that: the last ones inject nothing)
        out.append((f"upload fail_alloc={k}", "upload", {"GENPHI_TEST_FAIL_ALLOC": str(k)}, [_call(None), _call(None), _call((10, 20))]))
        out.append((f"upload wide fail_alloc={k}", "upload", {"GENPHI_TEST_FAIL_ALLOC": str(k), "GENPHI_LDS_CAP_FLOATS": "300"},
                    [_call((10, 20)), _call((10, 20)), _call(None)]))
    return out


def _run_case(gen, peds, ped_name, env, calls):
    from genlib_jl_amd import _capi
    saved = {k: os.environ.pop(k, None) for k in HOOKS}
    os.environ.update(env)
    try:
        if ped_name not in peds:
            ind, fa, mo, sex, pro = _ped(ped_name)
            peds[ped_name] = (gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}), pro)
        ped, pro = peds[ped_name]
        pl = gen.plan(ped, pro)
        n = pl.n_probands
        n_steps = len(pl.step_modes())
        rec = {"modes": pl.step_modes(), "last_slots": list(pl.step_slots(n_steps - 1)) if n_steps else [], "calls": []}
        for c in calls:
            rows = None if c["rows"] is None else tuple(n if r < 0 else r for r in c["rows"])
            f64 = c.get("storage64", False)
            r = {"error": None, "text": ""}
            try:
                st = pl.compute_device(rows=rows, kernel=c.get("kernel", 0), timing=c.get("timing", False), storage64=f64)
                host = pl.result_to_host_f64() if f64 else pl.result_to_host()
                r.update(n_steps=int(st.n_steps), level_rows=[int(st.level_rows[s]) for s in range(min(int(st.n_steps), len(st.level_rows)))],
                         shape=list(host.shape), sha256=hashlib.sha256(np.ascontiguousarray(host).tobytes()).hexdigest())
                if c.get("timing", False):
                    r["timed"] = int(st.timed)
            except (gen.GenphiDeviceError, ValueError, MemoryError) as e:
                r.update(error=type(e).__name__, text=str(e))
                assert str(e) == _capi.last_error()
            r["device_bytes"] = pl.device_bytes
            rec["calls"].append(r)
        pl.close()
        return rec
    finally:
        for k in HOOKS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def _run_all(gen):
    peds = {}
    return {name: _run_case(gen, peds, ped, env, calls) for name, ped, env, calls in _cases()}


@pytest.mark.gpu
def test_sweep_host_contract(gen):
    want = json.load(open(GOLDEN))
    got = _run_all(gen)
    assert sorted(got) == sorted(want)
    for name in want:
        assert len(got[name]["calls"]) == len(want[name]["calls"]), name
        for k, (g, w) in enumerate(zip(got[name]["calls"], want[name]["calls"])):
            assert g == w, (name, k)
        assert got[name] == want[name], name


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_sweep_host_contract.py --record    (on a GPU, from the build to pin)"
    os.environ["GENPHI_ENV_HOOKS"] = "1"
    sys.path.insert(0, os.path.dirname(HERE))
    import genlib_jl_amd
    with open(GOLDEN, "w") as f:
        json.dump(_run_all(genlib_jl_amd), f, indent=0, sort_keys=True)
        f.write("\n")
