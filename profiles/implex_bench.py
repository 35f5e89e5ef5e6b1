"""gen.implex on one GPU: device time of the sweep, its algorithmic bytes and the share of the HBM peak they give, in both modes.

    python profiles/implex_bench.py [--workload genea140|cfg3|cfg4 ...] [--reps 5] [--check] [--host-walk]

One JSON line per workload and mode (what = "implex" | "implex_only_new"):
  plan_ms (host: ImplexPlan, median of three), sweep_ms (median over --reps sweeps after one warm-up; HIP events around the sweep,
  genphi_implex_stats), algorithmic_bytes (sum over g of (|U_g| + child list entries of U_g) x words of a panel row x 8, over
  the panels), effective_gbs = algorithmic_bytes / sweep_ms, hbm_peak_share (of 8 TB/s), generations, panel_cols, panels,
  lanes_per_row, peak_rows, sum_rows (sum of |U_g|), and call_ms_IND / call_ms_MEAN: the wall time of gen.implex(..., type=)
  (median of --reps calls after a warm-up: plan, upload, sweep, copy, free).
--check compares every count with tests/implex_oracle.py's implex_frontier (cfg4: minutes of Python).
--host-walk times the per-proband set walk of tests/implex_oracle.py (implex_literal) on genea140, for scale.
Workloads: those of profiles/gc_bench.py (genea140 with its 140 probands, cfg3 = synth.random_mating(100_000, 10_000, 20),
cfg4 = the bench pedigree, 1e6 individuals / 1e5 probands).
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
    ped, pro, _ = load(name)
    arrs = (ped.ind, ped.father, ped.mother, pro)
    for only_new in (False, True):
        gen._capi.lib().genphi_release_cached()
        plans = []
        for r in range(3):
            t0 = time.perf_counter()
            h = gen.ImplexPlan(*arrs, only_new=only_new)
            plans.append((time.perf_counter() - t0) * 1e3)
            if r < 2:
                h.close()
        try:
            times = sweeps(h, args.reps)
            st = h.stats()
            ms = float(np.median(times))
            res = {"workload": name, "what": "implex_only_new" if only_new else "implex", "n_ind": len(ped), "n_pro": len(pro),
                   "generations": st["generations"], "plan_ms": round(float(np.median(plans)), 3), "sweep_ms": round(ms, 4),
                   "sweep_ms_all": [round(t, 4) for t in times], "algorithmic_bytes": st["algorithmic_bytes"],
                   "effective_gbs": round(st["algorithmic_bytes"] / ms / 1e6, 1),
                   "hbm_peak_share": round(st["algorithmic_bytes"] / ms / 1e6 / HBM_PEAK_GBS, 4), "panel_cols": st["panel_cols"],
                   "panels": st["panels"], "lanes_per_row": st["lanes_per_row"], "peak_rows": st["peak_rows"],
                   "sum_rows": int(h.rows_per_generation().sum())}
            if args.check:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                from implex_oracle import implex_frontier
                counts, _ = implex_frontier(*arrs, only_new=only_new)
                res["counts_equal_oracle"] = bool(np.array_equal(h.counts(), counts))
        finally:
            h.close()
        for type_ in ("IND", "MEAN"):
            walls = []
            for r in range(args.reps + 1):
                t0 = time.perf_counter()
                gen.implex(ped, pro, type=type_, onlyNewAnc=only_new, device=0)
                if r:
                    walls.append((time.perf_counter() - t0) * 1e3)
            res["call_ms_" + type_] = round(float(np.median(walls)), 3)
        print(json.dumps(res), flush=True)
    if args.host_walk and name == "genea140":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from implex_oracle import implex_literal
        t0 = time.perf_counter()
        implex_literal(*arrs)
        print(json.dumps({"workload": name, "what": "host_walk_python_sets", "ms": round((time.perf_counter() - t0) * 1e3, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["genea140", "cfg3", "cfg4"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--host-walk", action="store_true")
    args = ap.parse_args()
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
