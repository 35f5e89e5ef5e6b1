"""Gene dropping (gen.simuSample / gen.simuProb) on one GPU: device time of the sweep, its algorithmic bytes and the share of the
HBM peak they give.

    python profiles/simu_bench.py [--workload genea140|cfg3|cfg4 ...] [--simul 5000] [--reps 5] [--seed 7] [--check]

One JSON line per workload (what = "simu"): plan_ms (host: SimuPlan, median of three), sweep_ms (median over --reps sweeps after
one warm-up; HIP events around the sweep, genphi_simu_stats; the handle is created without a sample: the sweep, the state
counts), algorithmic_bytes (per live row above level 0: two parent rows read and one written, 32 bytes per pair of words, over
the panels), effective_gbs = algorithmic_bytes / sweep_ms, hbm_peak_share (of 8 TB/s), levels, n_live, panel_cols, panels,
lanes_per_row, match_ms (one genphi_simu_match_counts on the swept handle, wall), and call_ms_simuProb / call_ms_simuSample:
the wall time of a whole call (median of --reps calls after a warm-up: plan, upload, sweep, copy, free; simuSample is skipped
where the sample would exceed 2 GiB).
--check compares the state counts with tests/simu_oracle.py's vectorised reference (cfg4: minutes of numpy).
Workloads: those of profiles/gc_bench.py, the founders as ancestors with state 1.  GENPHI_ENV_HOOKS=1 GENPHI_SIMU_PANEL=<columns>
forces a panel width (the A/B for cache-sized panels).
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
    ped, pro, anc = load(name)
    states = np.ones(len(anc), dtype=np.int32)
    arrs = (ped.ind, ped.father, ped.mother, pro, anc, states)
    gen._capi.lib().genphi_release_cached()
    plans = []
    for r in range(3):
        t0 = time.perf_counter()
        h = gen.SimuPlan(*arrs, simul_no=args.simul, seed=args.seed, no_sample=True)
        plans.append((time.perf_counter() - t0) * 1e3)
        if r < 2:
            h.close()
    try:
        times = sweeps(h, args.reps)
        st = h.stats()
        ms = float(np.median(times))
        res = {"workload": name, "what": "simu", "n_ind": len(ped), "n_pro": len(pro), "n_anc": len(anc), "simul": args.simul,
               "levels": st["levels"], "n_live": st["n_live"], "plan_ms": round(float(np.median(plans)), 3), "sweep_ms": round(ms, 4),
               "sweep_ms_all": [round(t, 4) for t in times], "algorithmic_bytes": st["algorithmic_bytes"],
               "effective_gbs": round(st["algorithmic_bytes"] / ms / 1e6, 1) if ms else None,
               "hbm_peak_share": round(st["algorithmic_bytes"] / ms / 1e6 / HBM_PEAK_GBS, 4) if ms else None,
               "panel_cols": st["panel_cols"], "panels": st["panels"], "lanes_per_row": st["lanes_per_row"]}
        t0 = time.perf_counter()
        h.match_counts(np.ones(len(pro), dtype=np.int32))
        res["match_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        if args.check:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from simu_oracle import SimuVector, state_counts
            want = SimuVector(*arrs).sample(args.simul, args.seed)
            res["state_counts_equal_oracle"] = bool(np.array_equal(h.state_counts(), state_counts(want)))
    finally:
        h.close()
    calls = [("simuProb", lambda: gen.simuProb(ped, pro, np.ones(len(pro), dtype=np.int64), anc, states, simulNo=args.simul,
                                               seed=args.seed, device=0))]
    if len(pro) * args.simul <= 2 << 30:
        calls.append(("simuSample", lambda: gen.simuSample(ped, pro, anc, states, simulNo=args.simul, seed=args.seed, device=0)))
    for what, call in calls:
        walls = []
        for r in range(args.reps + 1):
            t0 = time.perf_counter()
            call()
            if r:
                walls.append((time.perf_counter() - t0) * 1e3)
        res["call_ms_" + what] = round(float(np.median(walls)), 3)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["genea140", "cfg3", "cfg4"])
    ap.add_argument("--simul", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
