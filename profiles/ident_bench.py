"""gen.simuIdentity on one GPU: device time of the label sweep and of the pair kernel, the pair kernel's word operations per second,
and one A/B of the pair kernel's two forms.

    python profiles/ident_bench.py [--workload genea140 synth2000 synth10000 ...] [--simul 5000] [--reps 5] [--seed 7]

One JSON line per workload (what = "ident"): plan_ms (host: IdentityPlan), sweep_ms and pair_ms (each the median over --reps
computes after one warm-up; HIP events, genphi_ident_stats: init and level steps / gather and pair kernel, summed over the panels),
algorithmic_bytes and effective_gbs of the sweep, word_ops (ordered pairs computed x words x (12 B + 40)) and word_gops =
word_ops / pair_ms, n_live, levels, n_labels, planes, the tile, panel_cols, panels; and the A/B on the same inputs:
pair_ms_all_pairs, the pair kernel computing every ordered pair (GENPHI_IDENT_FLAG_ALL_PAIRS) where the shipped form computes the
tiles on or above the diagonal and mirrors them, all_pairs_over_shipped = the ratio of the two medians, and counts_equal: the two
forms give the same bytes.
Workloads: genea140 (its 140 probands); synthN: synth.random_mating with N probands in the last of 10 generations of N each
(5 % of the parents drawn from two generations up).
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


def load(name):
    import genlib_jl_amd as gen
    from genlib_jl_amd import synth
    if name == "genea140":
        ped = gen.genealogy(gen.genea140)
        return ped, gen.pro(ped)
    n = int(name[len("synth"):])
    ind, fa, mo, sex, pro = synth.random_mating(10 * n, n, 10, skip_permille=50)
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}), np.ascontiguousarray(pro, dtype=np.int64)


def computes(h, reps):
    sweep, pair = [], []
    for r in range(reps + 1):
        h.compute(device=0)
        st = h.stats()
        if r:
            sweep.append(st["sweep_ms"])
            pair.append(st["pair_ms"])
    return sweep, pair, st


def run(name, args):
    import genlib_jl_amd as gen
    ped, pro = load(name)
    arrs = (ped.ind, ped.father, ped.mother, pro)
    gen._capi.lib().genphi_release_cached()
    t0 = time.perf_counter()
    h = gen.IdentityPlan(*arrs, simul_no=args.simul, seed=args.seed)
    plan_ms = (time.perf_counter() - t0) * 1e3
    try:
        sweep, pair, st = computes(h, args.reps)
        counts = h.counts_to_host()
        res = {"workload": name, "what": "ident", "n_ind": len(ped), "n_pro": len(pro), "simul": args.simul, "n_live": h.n_live,
               "levels": st["levels"], "n_labels": h.n_labels, "planes": st["planes"], "tile": [st["tile_rows"], st["tile_cols"]],
               "panel_cols": st["panel_cols"], "panels": st["panels"], "lanes_per_row": st["lanes_per_row"], "plan_ms": round(plan_ms, 3),
               "sweep_ms": round(float(np.median(sweep)), 4), "sweep_ms_all": [round(t, 4) for t in sweep],
               "pair_ms": round(float(np.median(pair)), 4), "pair_ms_all": [round(t, 4) for t in pair],
               "algorithmic_bytes": st["algorithmic_bytes"], "word_ops": st["word_ops"]}
        res["effective_gbs"] = round(st["algorithmic_bytes"] / res["sweep_ms"] / 1e6, 1) if res["sweep_ms"] else None
        res["word_gops"] = round(st["word_ops"] / res["pair_ms"] / 1e6, 1) if res["pair_ms"] else None
        res["sums_to_S"] = bool(np.all(counts.sum(axis=-1) == args.simul))
    finally:
        h.close()
    h = gen.IdentityPlan(*arrs, simul_no=args.simul, seed=args.seed, all_pairs=True)
    try:
        _, pair, st = computes(h, args.reps)
        res["pair_ms_all_pairs"] = round(float(np.median(pair)), 4)
        res["pair_ms_all_pairs_all"] = [round(t, 4) for t in pair]
        res["word_gops_all_pairs"] = round(st["word_ops"] / res["pair_ms_all_pairs"] / 1e6, 1) if res["pair_ms_all_pairs"] else None
        res["all_pairs_over_shipped"] = round(res["pair_ms_all_pairs"] / res["pair_ms"], 3) if res["pair_ms"] else None
        res["counts_equal"] = bool(np.array_equal(h.counts_to_host(), counts))
    finally:
        h.close()
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
