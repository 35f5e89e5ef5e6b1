"""gen.gc on one GPU: device time of the sweep, its algorithmic bytes and the effective bandwidth they give.

    python profiles/gc_bench.py [--workload genea140|cfg3|cfg4|cfg4_16 ...] [--reps 5]
                                [--panel C] [--cache-panels] [--check-rows N]

One JSON line per workload:
    sweep_ms          median over --reps sweeps after one warm-up (HIP events around the sweep, genphi_gc_stats)
    algorithmic_bytes for each computed row, its source rows read and its row written at 8 bytes per panel column, plus the
                      4-byte result
    effective_gbs     algorithmic_bytes / sweep_ms.  With panels sized for the Infinity Cache the source rows may be served
                      from it: this is an effective rate, not a fraction of HBM bandwidth (hbm_peak_gbs is given for scale)
    peak_slots, panel_cols, panels_per_launch, d2h_ms (one copy of the result to pageable host memory)
--panel C sets the panel width (GENPHI_GC_PANEL); --cache-panels sizes panels so that the live slot rows of one panel stay
within about 150 MiB (the 256 MiB Infinity Cache) and runs one panel per launch (GENPHI_GC_PANELS_PER_LAUNCH=1).
--check-rows N compares N sampled rows with the exact contributions (tests/gc_oracle.py).
Workloads: genea140 x all 7,399 founders; cfg3 (1e5 individuals, 1e4 probands, 20 generations) x all 6,633 founders;
cfg4 (1e6 individuals, 1e5 probands, 30 generations) x all 50,366 founders (a 20 GB result); cfg4 x 16 founders.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HBM_PEAK_GBS = 8000.0
CACHE_SLOT_BYTES = 150 << 20


def load(name):
    import genlib_jl_amd as gen
    from genlib_jl_amd import synth
    if name == "genea140":
        ped = gen.genealogy(gen.genea140)
        return ped, gen.pro(ped), gen.founder(ped)
    shape = {"cfg3": (100_000, 10_000, 20), "cfg4": (1_000_000, 100_000, 30), "cfg4_16": (1_000_000, 100_000, 30)}[name]
    ind, fa, mo, sex, pro = synth.random_mating(*shape)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    anc = gen.founder(ped)
    if name == "cfg4_16":
        anc = anc[np.random.default_rng(16).choice(len(anc), 16, replace=False)]
    return ped, pro, anc


def run(name, args):
    import genlib_jl_amd as gen
    ped, pro, anc = load(name)
    t0 = time.perf_counter()
    h = gen.GCPlan(ped.ind, ped.father, ped.mother, pro, anc)
    create_ms = (time.perf_counter() - t0) * 1e3
    if args.cache_panels:
        peak = h.stats()["peak_slots"]
        h.close()
        os.environ["GENPHI_GC_PANEL"] = str(max(1, CACHE_SLOT_BYTES // (8 * max(peak, 1))))
        os.environ["GENPHI_GC_PANELS_PER_LAUNCH"] = "1"
        h = gen.GCPlan(ped.ind, ped.father, ped.mother, pro, anc)
    try:
        times = []
        for r in range(args.reps + 1):
            h.compute(device=0)
            if r:
                times.append(h.stats()["sweep_ms"])
        st = h.stats()
        t0 = time.perf_counter()
        out = h.result_to_host()
        d2h_ms = (time.perf_counter() - t0) * 1e3
    finally:
        h.close()
    ms = float(np.median(times))
    res = {"workload": name, "n_pro": len(pro), "n_anc": len(anc), "result_bytes": int(out.nbytes), "create_ms": round(create_ms, 1),
           "sweep_ms": round(ms, 3), "sweep_ms_all": [round(t, 3) for t in times], "algorithmic_bytes": st["algorithmic_bytes"],
           "effective_gbs": round(st["algorithmic_bytes"] / ms / 1e6, 1), "hbm_peak_gbs": HBM_PEAK_GBS,
           "effective_over_peak": round(st["algorithmic_bytes"] / ms / 1e6 / HBM_PEAK_GBS, 3),
           "peak_slots": st["peak_slots"], "panel_cols": st["panel_cols"],
           "panels_per_launch": os.environ.get("GENPHI_GC_PANELS_PER_LAUNCH", "default"), "d2h_ms": round(d2h_ms, 1)}
    if args.check_rows:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from gc_oracle import gc_exact_rows
        sample = np.random.default_rng(1).choice(len(pro), min(args.check_rows, len(pro)), replace=False)
        ref = gc_exact_rows(ped.ind, ped.father, ped.mother, pro, anc, sample=sample)
        res["checked_rows"] = len(sample)
        res["rows_equal_exact"] = bool(np.array_equal(out[sample].view(np.int32), ref.view(np.int32)))
    res["row_sums_one"] = bool(np.all(out.sum(axis=1, dtype=np.float64) == 1.0))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["genea140", "cfg3", "cfg4", "cfg4_16"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--panel", type=int, default=0)
    ap.add_argument("--cache-panels", action="store_true")
    ap.add_argument("--check-rows", type=int, default=0)
    args = ap.parse_args()
    if args.panel:
        os.environ["GENPHI_GC_PANEL"] = str(args.panel)
    if args.panel or args.cache_panels:
        os.environ["GENPHI_ENV_HOOKS"] = "1"           # (read once, when the library loads)
    sys.path.insert(0, ROOT)
    for name in args.workload:
        print(json.dumps(run(name, args)), flush=True)


if __name__ == "__main__":
    main()
