"""The contract of the nine genphi_result_* entry points (include/genphi.h), recorded: every one called with valid arguments and with
each invalid argument the header documents, in every state a plan can be in, and (return code, genphi_last_error() text after a
failure, what the call left in its outputs) compared exactly with tests/golden/result_queries_contract.json.  The file was written
by record() below against a build of the commit BEFORE the queries left genphi_hip.hip (its package directory first on sys.path);
moving code must not change a code, a message or a value.  Outputs start from a sentinel, so what a call leaves untouched is part of
the record.  No call here makes an allocation fail: messages that embed allocation sizes are not recorded."""
import ctypes as C
import hashlib
import json
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "result_queries_contract.json")
I32P, I64P, F32P, F64P = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_double)
SENTINEL = -7


def _enc(a):
    """An array as JSON: its values (every float32 / float64 is exactly a Python float), or its digest when it is long."""
    a = np.ascontiguousarray(a)
    if a.size <= 64:
        return a.astype(np.float64).tolist() if a.dtype.kind == "f" else a.tolist()
    return {"dtype": str(a.dtype), "shape": list(a.shape), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


def _rec(gen, rc, outs):
    return {"rc": int(rc), "err": gen._capi.last_error() if rc else None, "out": {k: _enc(v) for k, v in outs.items()}}


def _arr(n, dtype):
    return np.full(max(int(n), 1), SENTINEL, dtype=dtype)


def _over(gen, h, t, cap, arrays=(True, True, True), want_n=True):
    """The record of one genphi_result_over call: threshold t, room for cap pairs, the arrays asked for."""
    L = gen._capi.lib()
    r, c, v, n = _arr(cap, np.int32), _arr(cap, np.int32), _arr(cap, np.float32), C.c_int64(SENTINEL)
    ptr = lambda a, on, t_: a.ctypes.data_as(t_) if on else None  # noqa: E731
    rc = L.genphi_result_over(h, t, cap, ptr(r, arrays[0], I32P), ptr(c, arrays[1], I32P), ptr(v, arrays[2], F32P), C.byref(n) if want_n else None)
    return _rec(gen, rc, {"rows": r, "cols": c, "values": v, "n_pairs": np.array([n.value])})


def _over_cache_calls(gen, h, N):
    """A count-only call, then a filling call, both at ONE threshold and nothing else: the offsets the plan keeps afterwards are
    those of this threshold and of the resident rows."""
    return {"over/count only": _over(gen, h, 2.0 ** -6, 0, (False, False, False)), "over/fill": _over(gen, h, 2.0 ** -6, N * (N - 1) // 2)}


def _calls(gen, h, N, r0, nr):
    """name -> record of every call on plan handle h (None = the NULL plan); N probands, resident rows [r0, r0 + nr) as far as the
    test knows (they only choose the arguments)."""
    L = gen._capi.lib()
    out = {}

    def p(a, t):
        return None if a is None else a.ctypes.data_as(t)

    # genphi_result_device
    ptr, ld, b, n = C.c_void_p(), C.c_int64(SENTINEL), C.c_int64(SENTINEL), C.c_int64(SENTINEL)
    rc = L.genphi_result_device(h, C.byref(ptr), C.byref(ld), C.byref(b), C.byref(n))
    out["device"] = _rec(gen, rc, {"has_ptr": np.array([bool(ptr.value)]), "ld_row_begin_n_rows": np.array([ld.value, b.value, n.value])})
    out["device/no outputs"] = _rec(gen, L.genphi_result_device(h, None, None, None, None), {})
    # genphi_result_to_host, genphi_result_to_host_f64
    for name, fn, dt, t in (("to_host", L.genphi_result_to_host, np.float32, F32P), ("to_host_f64", L.genphi_result_to_host_f64, np.float64, F64P)):
        a = _arr(nr * N, dt)
        out[name] = _rec(gen, fn(h, p(a, t)), {"out": a})
        out[name + "/out NULL"] = _rec(gen, fn(h, None), {})
    # genphi_result_sums
    sa, sd, n = C.c_double(SENTINEL), C.c_double(SENTINEL), C.c_int64(SENTINEL)
    rc = L.genphi_result_sums(h, C.byref(sa), C.byref(sd), C.byref(n))
    out["sums"] = _rec(gen, rc, {"sum_all_sum_diag": np.array([sa.value, sd.value]), "n_rows": np.array([n.value])})
    out["sums/no outputs"] = _rec(gen, L.genphi_result_sums(h, None, None, None), {})
    # genphi_result_group_sums: interleaved labels with an unlabelled proband (form 1), one run per group (form 0), one group
    def group_sums(name, g, labels, want=True):
        s, d, rg, cg, form = _arr(g * g, np.float64), _arr(g, np.float64), _arr(g, np.int64), _arr(g, np.int64), C.c_int32(SENTINEL)
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32)
        if want:
            rc = L.genphi_result_group_sums(h, g, p(lab, I32P), p(s, F64P), p(d, F64P), p(rg, I64P), p(cg, I64P), C.byref(form))
            out[name] = _rec(gen, rc, {"sums": s, "diag": d, "rows_in_group": rg, "cols_in_group": cg, "form": np.array([form.value])})
        else:
            out[name] = _rec(gen, L.genphi_result_group_sums(h, g, p(lab, I32P), None, None, None, None, None), {})
    k = np.arange(max(N, 1))
    inter = np.where(k % 5 == 4, -1, k % 3)
    group_sums("group_sums/interleaved", 3, inter)
    group_sums("group_sums/runs", 2, (k >= (N + 1) // 2).astype(np.int32))
    group_sums("group_sums/one group", 1, np.zeros_like(k))
    group_sums("group_sums/all unlabelled", 2, np.full_like(k, -1))
    group_sums("group_sums/no outputs", 3, inter, want=False)
    group_sums("group_sums/n_groups 0", 0, inter)
    group_sums("group_sums/n_groups 4097", 4097, inter, want=False)
    group_sums("group_sums/group NULL", 3, None)
    group_sums("group_sums/label -2", 3, np.where(k == k[-1], -2, inter))
    group_sums("group_sums/label n_groups", 3, np.where(k == 0, 3, inter))
    # genphi_result_over
    def over(name, *args, **kw):
        out[name] = _over(gen, h, *args, **kw)
    pairs = N * (N - 1) // 2
    over("over/count only", 2.0 ** -6, 0, (False, False, False))
    over("over/fill", 2.0 ** -6, pairs)
    over("over/every pair", -math.inf, pairs)
    over("over/cap too small", -math.inf, max(pairs - 1, 0))
    over("over/no pair", math.inf, pairs)
    over("over/values only", 0.0, pairs, (False, False, True), want_n=False)
    over("over/NaN", math.nan, pairs)
    over("over/cap -1", 0.0, -1)
    # genphi_result_nearest
    def nearest(name, kk, cols=True, values=True):
        c, v = _arr(nr * max(kk, 1), np.int32), _arr(nr * max(kk, 1), np.float32)
        rc = L.genphi_result_nearest(h, kk, p(c if cols else None, I32P), p(v if values else None, F32P))
        out[name] = _rec(gen, rc, {"cols": c, "values": v})
    nearest("nearest/k 1", 1)
    nearest("nearest/k max", min(N - 1, 64))
    nearest("nearest/cols only", 2, values=False)
    nearest("nearest/values only", 2, cols=False)
    nearest("nearest/both NULL", 1, cols=False, values=False)
    nearest("nearest/k 0", 0)
    nearest("nearest/k N", N)
    nearest("nearest/k 65", 65)
    # genphi_result_bootstrap
    def bootstrap(name, first, nb, quad=True, self_=True):
        q, s, n = _arr(nb, np.float64), _arr(nb, np.float64), C.c_int64(SENTINEL)
        rc = L.genphi_result_bootstrap(h, 20261018, first, nb, p(q if quad else None, F64P), p(s if self_ else None, F64P), C.byref(n))
        out[name] = _rec(gen, rc, {"quad": q, "self": s, "n_rows": np.array([n.value])})
    bootstrap("bootstrap", 0, 5)
    bootstrap("bootstrap/first 3", 3, 2)
    bootstrap("bootstrap/quad only", 0, 2, self_=False)
    bootstrap("bootstrap/no arrays", 0, 2, quad=False, self_=False)
    bootstrap("bootstrap/n_boot 0", 0, 0)
    bootstrap("bootstrap/first -1", -1, 1)
    bootstrap("bootstrap/first + n_boot 2^31", 2 ** 31 - 2, 2)
    # genphi_result_entries
    def entries(name, rows, cols, n=None, null=None):
        rows, cols = np.ascontiguousarray(rows, dtype=np.int64), np.ascontiguousarray(cols, dtype=np.int64)
        o = _arr(len(rows), np.float64)
        args = [p(rows, I64P), p(cols, I64P), p(o, F64P)]
        if null is not None:
            args[null] = None
        out[name] = _rec(gen, L.genphi_result_entries(h, len(rows) if n is None else n, *args), {"out": o})
    last = r0 + max(nr, 1) - 1
    entries("entries", [r0, last, last, r0], [0, N - 1, r0, last])
    entries("entries/n 0", [r0], [0], n=0)
    entries("entries/n -1", [r0], [0], n=-1)
    for which, name in enumerate(("rows", "cols", "out")):
        entries("entries/%s NULL" % name, [r0], [0], null=which)
    entries("entries/row below", [r0, r0 - 1], [0, 0])
    entries("entries/row above", [last + 1], [0])
    entries("entries/col -1", [r0], [-1])
    entries("entries/col N", [r0], [N])
    return out


def _pedigrees(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(400, 40, 5, skip_permille=50)
    return {"geneaJi": (gen.genealogy(gen.geneaJi), None, (1, 3)),
            "synthetic40": (gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}), pro, (7, 29))}


def record_cpu(gen):
    """The states that need no device: the NULL plan, a plan that never computed, a one-proband plan."""
    ped = gen.genealogy(gen.geneaJi)
    states = {"NULL plan": _calls(gen, None, 3, 0, 0)}
    for name, pro in (("never computed", None), ("one proband", [29])):
        pl = gen.plan(ped, pro)
        try:
            states[name] = _calls(gen, pl._h, pl.n_probands, 0, 0)
        finally:
            pl.close()
    return states


def record_gpu(gen, device=0):
    """Per pedigree: a full Float32 result, a row shard, an empty shard, a Float64 result, the plan after
    genphi_plan_release_device, and genphi_result_over counting, filling, and again after a recompute of other rows."""
    states = {}
    for ped_name, (ped, pro, shard) in _pedigrees(gen).items():
        pl = gen.plan(ped, pro)
        try:
            N = pl.n_probands
            for name, kw, r0, nr in (("full", {}, 0, N), ("shard", {"rows": shard}, shard[0], shard[1] - shard[0]), ("empty shard", {"rows": (2, 2)}, 2, 0),
                                     ("Float64", {"storage64": True}, 0, N)):
                pl.compute_device(device=device, **kw)
                states["%s/%s" % (ped_name, name)] = _calls(gen, pl._h, N, r0, nr)
            pl.release_device()
            states[ped_name + "/released"] = _calls(gen, pl._h, N, 0, 0)
            # Two shards of the same size, and in each nothing but a count and a fill at one threshold: when the second shard is
            # computed the plan holds offsets of that very threshold and of as many rows, so a cache that the recompute did not
            # drop would be taken for the new rows' -- the first shard's count and list would come back.
            half = N // 2
            for name, rows in (("over cache/first rows", (0, half)), ("over cache/other rows", (N - half, N))):
                pl.compute_device(device=device, rows=rows)
                states["%s/%s" % (ped_name, name)] = _over_cache_calls(gen, pl._h, N)
            first, other = (states["%s/over cache/%s rows" % (ped_name, w)] for w in ("first", "other"))
            assert first != other, "the two shards list the same pairs: the states cannot tell a kept cache from a dropped one"
        finally:
            pl.close()
    return states


def record(path=GOLDEN, gpu=True):
    """Writes the golden file from the genlib_jl_amd that sys.path finds; gpu=False keeps the file's recorded GPU states."""
    import genlib_jl_amd as gen
    old = json.load(open(path)) if os.path.exists(path) else {}
    doc = {"cpu": record_cpu(gen), "gpu": record_gpu(gen) if gpu else old.get("gpu", {})}
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)
        fh.write("\n")


def _compare(got, want):
    assert sorted(got) == sorted(want)
    for state in sorted(want):
        assert sorted(got[state]) == sorted(want[state]), state
        for call in sorted(want[state]):
            assert got[state][call] == want[state][call], (state, call, got[state][call], want[state][call])


def test_contract_without_a_device(gen):
    _compare(json.loads(json.dumps(record_cpu(gen))), json.load(open(GOLDEN))["cpu"])


@pytest.mark.gpu
def test_contract_on_the_device(gen):
    want = json.load(open(GOLDEN))["gpu"]
    assert want, "the golden file has no GPU states"
    _compare(json.loads(json.dumps(record_gpu(gen))), want)
