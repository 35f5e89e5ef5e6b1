"""Group sums of the resident kinship matrix on one GPU (genphi_result_group_sums) against the two routes that exist without it.

    python profiles/group_sums_bench.py [--workload cfg4|cfg3|cfg2k] [--groups 7 64 1000] [--reps 5] [--no-host-route]

One JSON line per (n_groups, form):
    ms, ms_all        median and all of --reps calls after one warm-up: host wall clock around PhiPlan.group_sums, which ends in
                      a stream synchronise (label checks, tables, upload, kernels, copy of the n_groups^2 table back: the call)
    ratio_to_sums     ms over the median of genphi_result_sums (row_sums_kernel: the same N^2 floats read once) taken the same
                      way on the same resident matrix, in the same process, alternating with the group calls
    spread            (max - min) / median of the repeats, for both
    effective_tbs     4 N^2 bytes / ms
    form 0: groups of equal size, each one run of the proband order; form 1: the same sizes, labels shuffled
and one line for the host route (unless --no-host-route): genphi_result_to_host + per-row np.add.reduceat + a group-by of the
rows, form 0 labels of the first --groups value; d2h_ms is the copy alone.
Workloads: cfg4 (1e6 individuals, 1e5 probands, 30 generations: a 40 GB matrix), cfg3 (1e5, 1e4, 20), cfg2k (3e4, 2.5e3, 10).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHAPES = {"cfg4": (1_000_000, 100_000, 30), "cfg3": (100_000, 10_000, 20), "cfg2k": (30_000, 2_500, 10)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(times):
    med = float(np.median(times))
    return {"ms": round(med, 3), "ms_all": [round(t, 3) for t in times], "spread": round((max(times) - min(times)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg4", choices=sorted(SHAPES))
    ap.add_argument("--groups", type=int, nargs="+", default=[7, 64, 1000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host-route", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import genlib_jl_amd as gen
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(*SHAPES[args.workload])
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    try:
        pl.compute_device(device=0)
        pl.compute_device(device=0)
        n = pl.n_probands
        nbytes = 4.0 * n * n
        total = None
        for g in args.groups:
            contiguous = (np.arange(n, dtype=np.int64) * g // n).astype(np.int32)
            shuffled = np.random.default_rng(g).permutation(contiguous)
            for form, labels in ((0, contiguous), (1, shuffled)):
                pl.group_sums(labels, g)
                pl.result_sums()
                t_group, t_sums = [], []
                for _ in range(args.reps):
                    ms, out = timed(lambda: pl.group_sums(labels, g))
                    t_group.append(ms)
                    ms, total = timed(pl.result_sums)
                    t_sums.append(ms)
                assert out[4] == form and abs(out[0].sum() - total[0]) <= 1e-9 * total[0] and abs(out[1].sum() - total[1]) <= 1e-9 * total[1]
                res = {"workload": args.workload, "n_pro": n, "n_groups": g, "form": form}
                res.update(summary(t_group))
                res["result_sums"] = summary(t_sums)
                res["ratio_to_sums"] = round(res["ms"] / res["result_sums"]["ms"], 3)
                res["effective_tbs"] = round(nbytes / res["ms"] / 1e9, 3)
                res["result_sums_tbs"] = round(nbytes / res["result_sums"]["ms"] / 1e9, 3)
                print(json.dumps(res), flush=True)
        if not args.no_host_route:
            g = args.groups[0]
            labels = (np.arange(n, dtype=np.int64) * g // n).astype(np.int32)
            starts = np.flatnonzero(np.diff(labels, prepend=-1))
            device = pl.group_sums(labels, g)[0]
            d2h_ms, phi = timed(pl.result_to_host)
            t0 = time.perf_counter()
            per_row = np.add.reduceat(phi, starts, axis=1, dtype=np.float64)
            host = np.add.reduceat(per_row, starts, axis=0)
            sum_ms = (time.perf_counter() - t0) * 1e3
            print(json.dumps({"workload": args.workload, "n_pro": n, "n_groups": g, "route": "result_to_host + numpy block sums",
                              "d2h_ms": round(d2h_ms, 1), "numpy_ms": round(sum_ms, 1), "ms": round(d2h_ms + sum_ms, 1),
                              "max_rel_diff_to_device": float(np.max(np.abs(host - device) / host))}), flush=True)
    finally:
        pl.close()


if __name__ == "__main__":
    main()
