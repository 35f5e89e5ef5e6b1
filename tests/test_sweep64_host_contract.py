"""The host side of a Float64-storage sweep (compute_device(storage64=True): gen.f, genphi_phi_pairs and the Float64 result queries run on
it), held to what it did while it was one function next to the Float32 sweep: for a fixed list of small plans and call sequences, the
outcome of every call (error class and text, stats.n_steps, every stats.level_rows[s], stats.timed of a timing call, whether stats.perm_ms
is 0, the plan's device bytes after the call, a SHA-256 of the host copy of the result) equals, with ==, what
tests/golden/sweep64_host_contract.json records.

The golden file was written by `python tests/test_sweep64_host_contract.py --record ROOT` on a GPU, ROOT being a checkout and build of the
commit BEFORE the Float64 sweep moved to csrc/sweep_f64.hip (ROOT goes first on sys.path, so its package directory and library are the
ones loaded): sharing the sweep's phases with the Float32 path must not change a code, a message, a count or a bit.  The Float32 calls
of the interleaved case must in addition give the hashes tests/golden/sweep_host_contract.json pins for the same plan and shard."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sweep64_host_contract.json")
GOLDEN32 = os.path.join(HERE, "golden", "sweep_host_contract.json")
HOOKS = ("GENPHI_LDS_CAP_FLOATS", "GENPHI_TEST_FAIL_ALLOC")

# "mating" has cuts of 680, 1350, 1574, 1379, 1189, 1009, 876, 827 and 900 members (pl.levels()); a Float64 source row of a cut of n
# members takes 8 * ((n + 2) // 2 * 2) bytes of LDS, and GENPHI_LDS_CAP_FLOATS = c allows 4 c bytes (csrc/f64_geometry.h).
CAP_ONE_ROW = 3200      # 12,800 bytes: one row of the widest cut (12,608) but not two -> split form (two rows of the first cut fit: full form)
CAP_NO_ROW = 1400       # 5,600 bytes: below one row of every cut but the first (5,456) -> per-entry form at kernel 0, split form in step 0
DEEP_SHARD = (3, 11)    # (shard A of "deep graph A A B A A" in the Float32 contract)


def _ped(name):
    from genlib_jl_amd import synth
    from test_sweep_host_contract import _ped as ped32
    if name == "lists":                  # (test_sparse_leading_cuts_float64) the calibration keeps at least two leading cuts as row lists
        return synth.random_mating(30000, 3000, 10, skip_permille=0)
    return ped32(name)


def _call(rows=None, f64=True, **kw):
    return dict(rows=rows, f64=f64, **kw)


def _cases():
    """(name, pedigree, environment hooks, calls).  A negative row counts from the number of probands."""
    out = []
    mating = [_call(None), _call((0, 1)), _call((131, 600)), _call((600, -1)), _call((7, 7)), _call(None, timing=True), _call(None, kernel=1),
              _call((131, 600), kernel=1, timing=True), _call(None, no_sparse=True), _call((131, 600), no_sparse=True, timing=True)]
    for cap in (None, CAP_ONE_ROW, CAP_NO_ROW):
        out.append((f"mating cap={cap}", "mating", {} if cap is None else {"GENPHI_LDS_CAP_FLOATS": str(cap)}, mating))
    out.append(("founders only", "founders", {}, [_call(None), _call((2, 5)), _call(None, timing=True), _call((2, 5), timing=True), _call((0, 1), kernel=1)]))
    A = DEEP_SHARD
    out.append(("deep interleaved", "deep", {}, [_call(A, f64=False), _call(A, f64=False), _call(A, f64=False), _call(A), _call(A, f64=False),
                                                 _call(A, timing=True), _call(A, f64=False)]))
    for k in range(1, 13):               # (one small upload makes fewer allocations than that: the last ones inject nothing)
        out.append((f"upload fail_alloc={k}", "upload", {"GENPHI_TEST_FAIL_ALLOC": str(k)}, [_call(None), _call(None), _call((10, 20))]))
    out.append(("leading cuts as row lists", "lists", {}, [_call((100, 400)), _call((100, 400), no_sparse=True), _call(None, timing=True),
                                                           _call(None, no_sparse=True), _call((2999, 3000))]))
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
        rec = {"modes": pl.step_modes(), "calls": []}
        for c in calls:
            rows = None if c["rows"] is None else tuple(n if r < 0 else r for r in c["rows"])
            r = {"error": None, "text": "", "f64": c["f64"]}
            try:
                st = pl.compute_device(rows=rows, kernel=c.get("kernel", 0), timing=c.get("timing", False), storage64=c["f64"],
                                       no_sparse=c.get("no_sparse", False))
                r.update(n_steps=int(st.n_steps), level_rows=[int(st.level_rows[s]) for s in range(min(int(st.n_steps), len(st.level_rows)))])
                if c["f64"]:
                    r["perm_ms_is_0"] = st.perm_ms == 0
                if c.get("timing", False):
                    r["timed"] = int(st.timed)
                host = pl.result_to_host_f64() if c["f64"] else pl.result_to_host()
                r.update(shape=list(host.shape), sha256=hashlib.sha256(np.ascontiguousarray(host).tobytes()).hexdigest())
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
def test_sweep64_host_contract(gen):
    want = json.load(open(GOLDEN))
    got = _run_all(gen)
    assert sorted(got) == sorted(want)
    for name in want:
        assert len(got[name]["calls"]) == len(want[name]["calls"]), name
        for k, (g, w) in enumerate(zip(got[name]["calls"], want[name]["calls"])):
            assert g == w, (name, k)
        assert got[name] == want[name], name
    # a Float64 call between Float32 ones disturbs neither the captured graph nor the resident result type: every Float32 call of the
    # interleaved case delivers the matrix the Float32 contract pins for this plan and shard
    pinned = json.load(open(GOLDEN32))["deep graph A A B A A"]["calls"][0]
    f32 = [c for c in got["deep interleaved"]["calls"] if not c["f64"]]
    assert len(f32) == 5 and pinned["error"] is None
    for c in f32:
        assert c["error"] is None and c["sha256"] == pinned["sha256"] and c["level_rows"] == pinned["level_rows"]
    # every Float64 call that succeeded: no delivery pass was timed, and a timing call with level steps was timed
    for name in got:
        for c, spec in zip(got[name]["calls"], next(x[3] for x in _cases() if x[0] == name)):
            if c["f64"] and c["error"] is None:
                assert c["perm_ms_is_0"] is True, name
                if spec.get("timing") and c["n_steps"] > 0 and c["shape"][0] > 0:
                    assert c["timed"] == 1, name


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: python tests/test_sweep64_host_contract.py --record ROOT    (on a GPU; ROOT: the build to pin)"
    os.environ["GENPHI_ENV_HOOKS"] = "1"
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.abspath(sys.argv[2]))
    import genlib_jl_amd
    assert os.path.dirname(os.path.abspath(genlib_jl_amd.__file__)).startswith(os.path.abspath(sys.argv[2]))
    with open(GOLDEN, "w") as f:
        json.dump(_run_all(genlib_jl_amd), f, indent=0, sort_keys=True)
        f.write("\n")
