"""gen.simuCarriers on one GPU: device time of the label sweep and of the count kernel, against gen.simuRetention's sweep and mark
kernel on the same inputs in the same process (the mark kernel decodes the same sides, with one bit instead of one dword per cell:
the yardstick), the A/B of the label chunks, and max_count = 8 against the full width.

    python profiles/carriers_bench.py [--workload genea140 synth2000 synth10000 ...] [--simul 5000] [--reps 5] [--seed 7]

One JSON line per workload (what = "carriers"): plan_ms (host: CarriersPlan), sweep_ms and count_ms of the default chunk (each the
median over --reps computes after one warm-up; HIP events, genphi_carry_stats: init and level steps / count kernel, summed over the
panels), count_ns_per_side_word = count_ms / (2 n x words of S x chunks), count_bytes and count_gbs, n_live, levels, n_labels,
planes, columns, chunk_labels, chunks, lds_bytes, panel_cols, panels; from gen.RetentionPlan on the same input: retain_sweep_ms,
retain_mark_ms, retain_chunks, mark_ns_per_side_word, count_over_mark (whole kernels) and count_over_mark_per_side (per decoded side
and word: the chunks differ); sweeps_agree: the sum over c >= 1 of carriers equals survived; the chunks: count_ms_chunk[128], [256],
[512] and [608] with chunks_equal; the width: count_ms_max8 and wall_ms_max8 against wall_ms_full (compute and the three copies to
the host), with max8_consistent: the lumped table is the full one with its tail summed.
Workloads: those of profiles/ident_bench.py; the listed probands are the cases, there are no controls.
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
from retain_bench import computes, med  # noqa: E402


def run(name, args):
    import genlib_jl_amd as gen
    ped, pro = load(name)
    arrs = (ped.ind, ped.father, ped.mother, pro)
    gen._capi.lib().genphi_release_cached()

    def measure(**kw):
        h = gen.CarriersPlan(*arrs, simul_no=args.simul, seed=args.seed, **kw)
        try:
            sweep, count, st = computes(h, args.reps, "count_ms")
            t0 = time.perf_counter()
            h.compute(device=0)
            out = h.carriers_to_host(), h.homozygotes_to_host(), h.excluded_to_host()
            wall = (time.perf_counter() - t0) * 1e3
            return sweep, count, st, out, h, wall
        finally:
            h.close()

    t0 = time.perf_counter()
    gen.CarriersPlan(*arrs, simul_no=args.simul, seed=args.seed).close()
    plan_ms = (time.perf_counter() - t0) * 1e3
    sweep, count, st, out, h, wall = measure()
    words = (args.simul + 63) // 64
    n = st["n_cases"]
    res = {"workload": name, "what": "carriers", "n_ind": len(ped), "n_cases": n, "simul": args.simul, "n_live": h.n_live, "levels": st["levels"],
           "n_labels": h.n_labels, "planes": st["planes"], "columns": st["columns"], "chunk_labels": st["chunk_labels"], "chunks": st["chunks"],
           "lds_bytes": st["lds_bytes"], "panel_cols": st["panel_cols"], "panels": st["panels"], "plan_ms": round(plan_ms, 3),
           "sweep_ms": med(sweep), "sweep_ms_all": [round(t, 4) for t in sweep], "count_ms": med(count), "count_ms_all": [round(t, 4) for t in count],
           "algorithmic_bytes": st["algorithmic_bytes"], "count_bytes": st["count_bytes"], "wall_ms_full": round(wall, 2)}
    res["count_gbs"] = round(st["count_bytes"] / res["count_ms"] / 1e6, 1) if res["count_ms"] else None
    res["count_ns_per_side_word"] = round(res["count_ms"] * 1e6 / (2 * n * words * st["chunks"]), 4)
    weight = np.arange(st["columns"], dtype=np.int64)
    res["invariant_sides"] = bool(int((out[0].astype(np.int64) @ weight).sum()) + int((out[1].astype(np.int64) @ weight).sum()) == 2 * n * args.simul)
    g = gen.RetentionPlan(*arrs, simul_no=args.simul, seed=args.seed)
    try:
        s, m, gs = computes(g, args.reps, "mark_ms")
        res["retain_sweep_ms"], res["retain_mark_ms"], res["retain_chunks"] = med(s), med(m), gs["chunks"]
        res["mark_ns_per_side_word"] = round(res["retain_mark_ms"] * 1e6 / (2 * len(pro) * words * gs["chunks"]), 4)
        res["sweeps_agree"] = bool(np.array_equal(out[0][:, 1:].sum(axis=1, dtype=np.int64), g.survived_to_host()))
    finally:
        g.close()
    res["count_over_mark"] = round(res["count_ms"] / res["retain_mark_ms"], 3) if res["retain_mark_ms"] else None
    res["count_over_mark_per_side"] = round(res["count_ns_per_side_word"] / res["mark_ns_per_side_word"], 3) if res["mark_ns_per_side_word"] else None
    res["count_ms_chunk"], res["chunks_forced"], equal = {}, {}, True
    for lc in (128, 256, 512, 608):
        _, c, s2, o, _, _ = measure(chunk_labels=lc)
        res["count_ms_chunk"][str(lc)] = med(c)
        res["chunks_forced"][str(lc)] = s2["chunks"]
        equal = equal and all(np.array_equal(a, b) for a, b in zip(out, o))
    res["chunks_equal"] = equal
    _, c, s2, o, _, wall8 = measure(max_count=8)
    res["count_ms_max8"], res["wall_ms_max8"], res["columns_max8"] = med(c), round(wall8, 2), s2["columns"]
    res["max8_consistent"] = bool(all(np.array_equal(a[:, :8], b[:, :8]) and np.array_equal(a[:, 8], b[:, 8:].sum(axis=1)) for a, b in zip(o[:2], out[:2])))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["genea140", "synth2000", "synth10000"])
    ap.add_argument("--simul", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
