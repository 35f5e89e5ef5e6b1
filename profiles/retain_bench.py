"""gen.simuRetention on one GPU: device time of the label sweep and of the mark kernel, the mark kernel's time per side and word, the
A/B of the two forms of its mark phase, the default label chunk against forced ones, and gen.simuIdentity on the same inputs in the
same process as the yardstick.

    python profiles/retain_bench.py [--workload genea140 synth2000 synth10000 ...] [--simul 5000] [--reps 5] [--seed 7] [--no-ident]

One JSON line per workload (what = "retain"): plan_ms (host: RetentionPlan), sweep_ms and mark_ms of the shipped form (each the
median over --reps computes after one warm-up; HIP events, genphi_retain_stats: init and level steps / mark kernel, summed over the
panels), mark_ns_per_side_word = mark_ms / (2 n_pro x words of S x chunks), algorithmic_bytes and effective_gbs of the sweep,
mark_bytes and mark_gbs, n_live, levels, n_labels, planes, chunk_labels, chunks, lds_bytes, panel_cols, panels; the A/B on the same
inputs: mark_ms_or (unconditional LDS atomic OR) and mark_ms_test (read the word first, skip the atomic when the bit is set),
test_over_or, and forms_equal: the two give the same bytes; the chunks: mark_ms_chunk[4096], [8192] and [16384] beside the default,
with chunks_equal; and from gen.IdentityPlan on the same input (unless --no-ident): ident_sweep_ms, the same label sweep, and
ident_pair_ms, gather + pair kernel, the cost of the only other route to the labels on the device.
Workloads: those of profiles/ident_bench.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from ident_bench import load  # noqa: E402


def computes(h, reps, second):
    sweep, other = [], []
    for r in range(reps + 1):
        h.compute(device=0)
        st = h.stats()
        if r:
            sweep.append(st["sweep_ms"])
            other.append(st[second])
    return sweep, other, st


def med(x):
    return round(float(np.median(x)), 4)


def run(name, args):
    import genlib_jl_amd as gen
    ped, pro = load(name)
    arrs = (ped.ind, ped.father, ped.mother, pro)
    gen._capi.lib().genphi_release_cached()

    def measure(**kw):
        h = gen.RetentionPlan(*arrs, simul_no=args.simul, seed=args.seed, **kw)
        try:
            sweep, mark, st = computes(h, args.reps, "mark_ms")
            return sweep, mark, st, (h.survived_to_host(), h.both_to_host(), h.distinct_to_host()), h
        finally:
            h.close()

    t0 = time.perf_counter()
    gen.RetentionPlan(*arrs, simul_no=args.simul, seed=args.seed).close()
    plan_ms = (time.perf_counter() - t0) * 1e3
    sweep, mark, st, out, h = measure()
    words = (args.simul + 63) // 64
    res = {"workload": name, "what": "retain", "n_ind": len(ped), "n_pro": len(pro), "simul": args.simul, "n_live": h.n_live, "levels": st["levels"],
           "n_labels": h.n_labels, "planes": st["planes"], "chunk_labels": st["chunk_labels"], "chunks": st["chunks"], "lds_bytes": st["lds_bytes"],
           "panel_cols": st["panel_cols"], "panels": st["panels"], "lanes_per_row": st["lanes_per_row"], "plan_ms": round(plan_ms, 3),
           "sweep_ms": med(sweep), "sweep_ms_all": [round(t, 4) for t in sweep], "mark_ms": med(mark), "mark_ms_all": [round(t, 4) for t in mark],
           "algorithmic_bytes": st["algorithmic_bytes"], "mark_bytes": st["mark_bytes"]}
    res["effective_gbs"] = round(st["algorithmic_bytes"] / res["sweep_ms"] / 1e6, 1) if res["sweep_ms"] else None
    res["mark_gbs"] = round(st["mark_bytes"] / res["mark_ms"] / 1e6, 1) if res["mark_ms"] else None
    res["mark_ns_per_side_word"] = round(res["mark_ms"] * 1e6 / (2 * len(pro) * words * st["chunks"]), 4)
    res["distinct_mean"] = round(float(out[2].mean()), 3)
    res["invariant_sums"] = bool(int(out[2].sum(dtype=np.int64)) == int(out[0].sum(dtype=np.int64)))
    forms = {}
    for form in ("or", "test"):
        _, m, _, o, _ = measure(mark=form)
        res["mark_ms_" + form] = med(m)
        res["mark_ms_%s_all" % form] = [round(t, 4) for t in m]
        forms[form] = o
    res["test_over_or"] = round(res["mark_ms_test"] / res["mark_ms_or"], 3) if res["mark_ms_or"] else None
    res["forms_equal"] = all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(out, forms["or"], forms["test"]))
    res["mark_ms_chunk"], res["chunks_forced"], equal = {}, {}, True
    for lc in (4096, 8192, 16384):
        _, m, s2, o, _ = measure(chunk_labels=lc)
        res["mark_ms_chunk"][str(lc)] = med(m)
        res["chunks_forced"][str(lc)] = s2["chunks"]
        equal = equal and all(np.array_equal(a, b) for a, b in zip(out, o))
    res["chunks_equal"] = equal
    if not args.no_ident:
        g = gen.IdentityPlan(*arrs, simul_no=args.simul, seed=args.seed)
        try:
            s, p, _ = computes(g, args.reps, "pair_ms")
            res["ident_sweep_ms"], res["ident_sweep_ms_all"], res["ident_pair_ms"] = med(s), [round(t, 4) for t in s], med(p)
        finally:
            g.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["genea140", "synth2000", "synth10000"])
    ap.add_argument("--simul", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--no-ident", action="store_true")
    args = ap.parse_args()
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
