"""gen.completeness on one GPU: device time of the sweep, its algorithmic bytes and the effective bandwidth they give, next to the
yardstick it is held against: gen.occ with 64-bit rows and as many ancestor columns as completeness has generations.

    python profiles/completeness_bench.py [--workload genea140|cfg3|cfg4 ...] [--reps 5] [--check]

Two JSON lines per workload, in the form of profiles/occ_bench.py:
  what = "completeness"   plan_ms (host: CompletenessPlan), sweep_ms (median over --reps sweeps after one warm-up; HIP events around
                          the sweep, genphi_comp_stats), algorithmic_bytes (8 G per source row read and slot row written, plus the
                          counts and percentages of the result), effective_gbs = algorithmic_bytes / sweep_ms, hbm_peak_share (of
                          8 TB/s), rows_moved (source rows read + slot rows written), us_per_launch, launches, peak_slots,
                          generations, and call_ms_IND / call_ms_MEAN: the wall time of gen.completeness(ped, pro, type="IND") and
                          of "MEAN" (median of --reps calls after a warm-up: plan, upload, sweep, copy, free)
  what = "occ64"          OccPlan(rows64=True) on the same pedigree and probands with G founders as ancestors: anc_step_kernel moves
                          the same bytes per row.  It computes only the rows that descend from one of those founders, so the figures
                          to compare are effective_gbs and the time per launch, not sweep_ms.
--check compares every entry of the completeness result with tests/completeness_oracle.py (not for cfg4: minutes of Python).
Workloads: those of profiles/gc_bench.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from occ_bench import sweeps  # noqa: E402

HBM_PEAK_GBS = 8000.0


def run(name, args):
    import genlib_jl_amd as gen
    from gc_bench import load
    ped, pro, founders = load(name)
    arrs = (ped.ind, ped.father, ped.mother, pro)
    gen._capi.lib().genphi_release_cached()
    plans = []
    for r in range(3):
        t0 = time.perf_counter()
        h = gen.CompletenessPlan(*arrs)
        plans.append((time.perf_counter() - t0) * 1e3)
        if r < 2:
            h.close()
    try:
        G = h.generations
        times = sweeps(h, args.reps)
        st = h.stats()
        ms = float(np.median(times))
        result_bytes = 16.0 * G * len(pro)
        rows = (st["algorithmic_bytes"] - result_bytes) / (8.0 * G)          # source rows read + slot rows written
        res = {"workload": name, "what": "completeness", "n_ind": len(ped), "n_pro": len(pro), "generations": G,
               "plan_ms": round(float(np.median(plans)), 3), "sweep_ms": round(ms, 4), "sweep_ms_all": [round(t, 4) for t in times],
               "algorithmic_bytes": st["algorithmic_bytes"], "effective_gbs": round(st["algorithmic_bytes"] / ms / 1e6, 1),
               "hbm_peak_share": round(st["algorithmic_bytes"] / ms / 1e6 / HBM_PEAK_GBS, 4), "rows_moved": int(rows),
               "us_per_launch": round(1e3 * ms / max(st["launches"], 1), 2), "launches": st["launches"],
               "peak_slots": st["peak_slots"], "row_entries": st["row_entries"]}
        if args.check:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from completeness_oracle import completeness_exact
            counts, _ = completeness_exact(*arrs)
            res["counts_equal_exact"] = bool(np.array_equal(h.counts(), counts))
    finally:
        h.close()
    for type_ in ("IND", "MEAN"):
        walls = []
        for r in range(args.reps + 1):
            t0 = time.perf_counter()
            gen.completeness(ped, pro, type=type_, device=0)
            if r:
                walls.append((time.perf_counter() - t0) * 1e3)
        res["call_ms_" + type_] = round(float(np.median(walls)), 3)
    print(json.dumps(res), flush=True)

    anc = founders[:G]
    o = gen.OccPlan(ped.ind, ped.father, ped.mother, pro, anc, rows64=True)
    try:
        times = sweeps(o, args.reps)
        st = o.stats()
        ms = float(np.median(times))
        print(json.dumps({"workload": name, "what": "occ64", "n_pro": len(pro), "n_anc": len(anc), "sweep_ms": round(ms, 4),
                          "sweep_ms_all": [round(t, 4) for t in times], "algorithmic_bytes": st["algorithmic_bytes"],
                          "effective_gbs": round(st["algorithmic_bytes"] / ms / 1e6, 1),
                          "us_per_launch": round(1e3 * ms / max(st["launches"], 1), 2), "launches": st["launches"],
                          "peak_slots": st["peak_slots"], "row_bits": st["row_bits"]}), flush=True)
    finally:
        o.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["genea140", "cfg3", "cfg4"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
