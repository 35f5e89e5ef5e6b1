"""gen.simuSharing on one GPU: device time of the linked-locus sweep and of the pair kernel, Philox blocks and algorithmic bytes per
second of the sweep, the pair kernel's word operations per second, the A/B of the pair kernel's two forms, and gen.simuIdentity's
pair kernel on the same probands at the same number of words, in the same process.

    python profiles/link_bench.py [--workload genea140 synth2000 synth10000 ...] [--loci 1024] [--length 1.0] [--simul 1000] [--reps 5] [--seed 7]

One JSON line per workload (what = "link"): plan_ms (host: SharingPlan), sweep_ms and pair_ms (each the median over --reps computes
after one warm-up; HIP events, genphi_link_stats: init and level steps / gather and pair kernel, summed over the panels), q,
philox_blocks and philox_gblocks = philox_blocks / sweep_ms, algorithmic_bytes and effective_gbs of the sweep, word_ops and word_gops =
word_ops / pair_ms, n_live, levels, n_labels, planes, the tile, panel_sims, panels, lanes_per_sim; the A/B on the same inputs:
pair_ms_all_pairs (GENPHI_LINK_FLAG_ALL_PAIRS: every tile, where the shipped form computes the tiles on or above the diagonal and
mirrors them), all_pairs_over_shipped and sums_equal; and ident_*: gen.IdentityPlan on the same probands with simul_no = simul x
loci, so that its pair kernel walks the same number of words: ident_pair_ms, ident_word_ops, ident_word_gops, and
link_over_ident_per_word_op = (pair_ms / word_ops) / (ident_pair_ms / ident_word_ops).
The word operations of a pair and word: gen.simuIdentity counts 12 B + 40 (six inequality words over B planes, then its state words
and eight popcounts); gen.simuSharing counts 8 B + 32: an XOR and an OR per plane for each of the four equality words ac, ad, bc, bd
(8 B), 8 to negate and mask them, 6 for any and two, 12 for the six popcounts (four into m, n1, n2) and their adds, and 6 for the
run count (shift, OR, AND-NOT, popcount, add, the carry).
Workloads: those of profiles/ident_bench.py: genea140 (its 140 probands); synthN: synth.random_mating with N probands in the last of
10 generations of N each (5 % of the parents drawn from two generations up).  --no-ident leaves the gen.simuIdentity run out.
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

from ident_bench import computes, load  # noqa: E402


def run(name, args):
    import genlib_jl_amd as gen
    ped, pro = load(name)
    arrs = (ped.ind, ped.father, ped.mother, pro)
    q = gen.sharing_q(args.loci, args.length)
    gen._capi.lib().genphi_release_cached()
    t0 = time.perf_counter()
    h = gen.SharingPlan(*arrs, loci=args.loci, q=q, simul_no=args.simul, seed=args.seed)
    plan_ms = (time.perf_counter() - t0) * 1e3
    try:
        sweep, pair, st = computes(h, args.reps)
        print("%s: shipped form done" % name, file=sys.stderr, flush=True)
        sums = h.sums_to_host()
        res = {"workload": name, "what": "link", "n_ind": len(ped), "n_pro": len(pro), "loci": args.loci, "length": args.length, "q": q,
               "simul": args.simul, "n_live": h.n_live, "levels": st["levels"], "n_labels": h.n_labels, "planes": st["planes"],
               "tile": [st["tile_rows"], st["tile_cols"]], "panel_sims": st["panel_sims"], "panels": st["panels"], "lanes_per_sim": st["lanes_per_sim"],
               "plan_ms": round(plan_ms, 3), "sweep_ms": round(float(np.median(sweep)), 4), "sweep_ms_all": [round(t, 4) for t in sweep],
               "pair_ms": round(float(np.median(pair)), 4), "pair_ms_all": [round(t, 4) for t in pair],
               "philox_blocks": st["philox_blocks"], "algorithmic_bytes": st["algorithmic_bytes"], "word_ops": st["word_ops"]}
        res["philox_gblocks"] = round(st["philox_blocks"] / res["sweep_ms"] / 1e6, 2) if res["sweep_ms"] else None
        res["effective_gbs"] = round(st["algorithmic_bytes"] / res["sweep_ms"] / 1e6, 1) if res["sweep_ms"] else None
        res["word_gops"] = round(st["word_ops"] / res["pair_ms"] / 1e6, 1) if res["pair_ms"] else None
        k = np.arange(len(pro))
        res["diagonal_ok"] = bool(np.all(sums[k, k, 2] == args.simul * args.loci) and np.all(sums[k, k, 4] == args.simul))
        res["symmetric"] = bool(np.array_equal(sums, sums.transpose(1, 0, 2)))
    finally:
        h.close()
    h = gen.SharingPlan(*arrs, loci=args.loci, q=q, simul_no=args.simul, seed=args.seed, all_pairs=True)
    try:
        _, pair, st = computes(h, args.reps)
        print("%s: every tile done" % name, file=sys.stderr, flush=True)
        res["pair_ms_all_pairs"] = round(float(np.median(pair)), 4)
        res["pair_ms_all_pairs_all"] = [round(t, 4) for t in pair]
        res["word_gops_all_pairs"] = round(st["word_ops"] / res["pair_ms_all_pairs"] / 1e6, 1) if res["pair_ms_all_pairs"] else None
        res["all_pairs_over_shipped"] = round(res["pair_ms_all_pairs"] / res["pair_ms"], 3) if res["pair_ms"] else None
        res["sums_equal"] = bool(np.array_equal(h.sums_to_host(), sums))
    finally:
        h.close()
    if not args.no_ident:
        h = gen.IdentityPlan(*arrs, simul_no=args.simul * args.loci, seed=args.seed)
        try:
            sweep, pair, st = computes(h, args.reps)
            res["ident_simul"] = args.simul * args.loci
            res["ident_panels"] = st["panels"]
            res["ident_sweep_ms"] = round(float(np.median(sweep)), 4)
            res["ident_pair_ms"] = round(float(np.median(pair)), 4)
            res["ident_pair_ms_all"] = [round(t, 4) for t in pair]
            res["ident_word_ops"] = st["word_ops"]
            res["ident_word_gops"] = round(st["word_ops"] / res["ident_pair_ms"] / 1e6, 1) if res["ident_pair_ms"] else None
            if res["pair_ms"] and res["ident_pair_ms"]:
                res["link_over_ident_per_word_op"] = round((res["pair_ms"] / res["word_ops"]) / (res["ident_pair_ms"] / st["word_ops"]), 3)
                res["link_over_ident_pair_ms"] = round(res["pair_ms"] / res["ident_pair_ms"], 3)
        finally:
            h.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["genea140", "synth2000", "synth10000"])
    ap.add_argument("--loci", type=int, default=1024)
    ap.add_argument("--length", type=float, default=1.0)
    ap.add_argument("--simul", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--no-ident", action="store_true")
    args = ap.parse_args()
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
