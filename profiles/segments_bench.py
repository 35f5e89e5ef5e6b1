"""gen.simuSegments on one GPU: device time of the segment kernel (link_segment_kernel, csrc/link.hip) beside the pair kernel of the
same compute, for three requests, in one process.

    python profiles/segments_bench.py [--workload genea140 synth2000 synth10000 ...] [--loci 1024] [--length 1.0] [--simul 1000] [--reps 5] [--seed 7]

One JSON line per workload (what = "segments").  Per request the median over --reps computes after one warm-up of segment_ms and of
pair_ms (HIP events, genphi_seg_stats and genphi_link_stats, summed over the panels), their ratio, the cells, the dynamic LDS of a
workgroup and the segments closed:
    bins      the default edges 1, 2, 4, .. alone (one pair of groups)
    groups7   the default edges and 7 groups (28 pairs of groups; every seventh list position in one group)
    cells     the largest table that can be asked for: 11 groups and 30 edges, 2,046 cells (G (G + 1) / 2 x (bins + 2) is never 2,048
              for 2 .. 257 edges)
and none: sweep_ms and pair_ms of the same handle with no request (the code path of profiles/link_bench.py).  Workloads: those of
profiles/link_bench.py.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from ident_bench import load  # noqa: E402


def computes(h, reps):
    seg, pair, sweep = [], [], []
    for r in range(reps + 1):
        h.compute(device=0)
        st, ss = h.stats(), h.segment_stats()
        if r:
            seg.append(ss["segment_ms"])
            pair.append(st["pair_ms"])
            sweep.append(st["sweep_ms"])
    return seg, pair, sweep, st, ss


def run(name, args):
    import genlib_jl_amd as gen
    from genlib_jl_amd import _segment_edges
    ped, pro = load(name)
    q = gen.sharing_q(args.loci, args.length)
    n = len(pro)
    default = _segment_edges(None, args.loci)
    wide = np.unique(np.round(np.geomspace(1, args.loci + 1, 60)).astype(np.int64))
    wide = wide[np.round(np.linspace(0, len(wide) - 1, 30)).astype(np.int64)]            # 30 strictly increasing edges from 1 to loci + 1
    requests = [("bins", default, None), ("groups7", default, np.arange(n) % 7), ("cells", wide, np.arange(n) % 11)]
    gen._capi.lib().genphi_release_cached()
    h = gen.SharingPlan(ped.ind, ped.father, ped.mother, pro, loci=args.loci, q=q, simul_no=args.simul, seed=args.seed)
    res = {"workload": name, "what": "segments", "n_pro": n, "loci": args.loci, "q": q, "simul": args.simul, "planes": h.planes}
    try:
        _, pair, sweep, st, _ = computes(h, args.reps)
        res["none"] = {"sweep_ms": round(float(np.median(sweep)), 4), "pair_ms": round(float(np.median(pair)), 4), "pair_ms_all": [round(t, 4) for t in pair]}
        res["panels"], res["panel_sims"] = st["panels"], st["panel_sims"]
        print("%s: no request done" % name, file=sys.stderr, flush=True)
        sums = h.sums_to_host()
        for key, edges, groups in requests:
            h.request_segments(edges, 1, groups)
            seg, pair, sweep, st, ss = computes(h, args.reps)
            hist, pairs = h.segments_to_host()
            up = np.triu_indices(n, 1)
            G = hist.shape[0]
            upper = np.triu(np.ones((G, G), dtype=bool))
            res[key] = {"segment_ms": round(float(np.median(seg)), 4), "segment_ms_all": [round(t, 4) for t in seg],
                        "pair_ms": round(float(np.median(pair)), 4), "sweep_ms": round(float(np.median(sweep)), 4),
                        "segment_over_pair": round(float(np.median(seg)) / float(np.median(pair)), 3) if np.median(pair) else None,
                        "cells": ss["cells"], "lds_bytes": ss["lds_bytes"], "segments": ss["segments"], "panels": st["panels"],
                        "word_gops": round(ss["word_ops"] / float(np.median(seg)) / 1e6, 1) if np.median(seg) else None,
                        "pairs_match_sums": bool(np.array_equal(pairs[..., 0], sums[..., 4]) and np.array_equal(pairs[..., 1], sums[..., 2])),
                        "table_matches_sums": bool(hist[upper][..., 0].sum() == sums[..., 4][up].sum() and hist[upper][..., 1].sum() == sums[..., 2][up].sum()),
                        "sums_unchanged": bool(np.array_equal(h.sums_to_host(), sums))}
            print("%s: %s done" % (name, key), file=sys.stderr, flush=True)
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
    args = ap.parse_args()
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
