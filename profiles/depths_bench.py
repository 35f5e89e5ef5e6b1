"""gen.depths on one GPU beside its two neighbours: device time of the sweep, its algorithmic bytes, and the time per byte against
gen.occ with 64-bit rows (the same recursion shape at half the element size) and gen.meioses, on the same inputs in the same process.

    python profiles/depths_bench.py [--workload genea140|cfg3|cfg4|cfg4_16 ...] [--by pair proband ancestor] [--reps 5]
                                    [--panel C] [--panels-per-launch G] [--check-rows N]

One JSON line per workload and quantity (what = "depths pair" / "depths proband" / "depths ancestor", "occ64", "meioses"), in the form
of profiles/occ_bench.py:
    sweep_ms          median over --reps sweeps after one warm-up (HIP events around the sweep, genphi_*_stats)
    algorithmic_bytes for each computed row, its source rows read and its row written (depths: 16 bytes per panel column), plus the
                      result entries (depths pair: 20 bytes each; the reductions: 20 per entry and 24 per accumulator)
    effective_gbs     algorithmic_bytes / sweep_ms: an effective rate (panels are sized for the Infinity Cache), not a share of HBM
                      bandwidth
    ps_per_byte       sweep_ms / algorithmic_bytes, in picoseconds
    peak_slots, panel_cols, launches, device_bytes (hipMemGetInfo before create and after the first compute)
then one line what = "ratios": ps_per_byte of each depths mode over that of occ64 and of meioses.  The expectation is a cost in
proportion to the bytes (a ratio near 1); the 20-byte result stream of the last list and the unpack make it somewhat larger.
--panel C / --panels-per-launch G: genphi_depth_create's panel_cols / panels_per_launch (0 = the default rule).  --check-rows N compares
N sampled proband rows of the pair result with depths_exact of tests/depths_oracle.py.  Workloads: those of profiles/gc_bench.py.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from occ_bench import free_bytes, sweeps  # noqa: E402


def report(name, what, n_pro, n_anc, h, times, used):
    st = h.stats()
    ms = float(np.median(times))
    return {"workload": name, "what": what, "n_pro": n_pro, "n_anc": n_anc, "sweep_ms": round(ms, 3), "sweep_ms_all": [round(t, 3) for t in times],
            "algorithmic_bytes": st["algorithmic_bytes"], "effective_gbs": round(st["algorithmic_bytes"] / ms / 1e6, 1),
            "ps_per_byte": round(ms * 1e9 / st["algorithmic_bytes"], 4), "peak_slots": st["peak_slots"], "panel_cols": st["panel_cols"],
            "launches": st["launches"], "device_bytes": int(used)}


def measure(gen, name, what, make, n_pro, n_anc, reps):
    gen._capi.lib().genphi_release_cached()
    before = free_bytes()
    h = make()
    try:
        h.compute(device=0)
        used = before - free_bytes()
        return report(name, what, n_pro, n_anc, h, sweeps(h, reps), used), h
    except BaseException:
        h.close()
        raise


def run(name, args):
    import genlib_jl_amd as gen
    from gc_bench import load
    ped, pro, anc = load(name)
    arrs = (ped.ind, ped.father, ped.mother, pro, anc)
    per_byte = {}
    for by in args.by:
        res, h = measure(gen, name, "depths " + by,
                         lambda: gen.DepthPlan(*arrs, by=by, panel_cols=args.panel, panels_per_launch=args.panels_per_launch), len(pro), len(anc), args.reps)
        try:
            if by == "pair" and args.check_rows:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                from depths_oracle import depths_exact
                sample = np.random.default_rng(1).choice(len(pro), min(args.check_rows, len(pro)), replace=False)
                ref = depths_exact(ped.ind, ped.father, ped.mother, pro[sample], anc)
                lo, hi, paths, mean = (a[sample] for a in h.result_to_host())
                res["checked_rows"] = len(sample)
                res["rows_equal_exact"] = bool(np.array_equal(lo, ref.min) and np.array_equal(hi, ref.max) and np.array_equal(paths, ref.paths) and
                                               np.array_equal(mean, ref.mean, equal_nan=True))
        finally:
            h.close()
        per_byte["depths " + by] = res["ps_per_byte"]
        print(json.dumps(res), flush=True)
    for what, make in (("occ64", lambda: gen.OccPlan(*arrs, rows64=True)), ("meioses", lambda: gen.DistPlan(*arrs))):
        res, h = measure(gen, name, what, make, len(pro), len(anc), args.reps)
        h.close()
        per_byte[what] = res["ps_per_byte"]
        print(json.dumps(res), flush=True)
    print(json.dumps({"workload": name, "what": "ratios",
                      **{"%s / %s" % (k, ref): round(v / per_byte[ref], 3) for k, v in per_byte.items() if k.startswith("depths")
                         for ref in ("occ64", "meioses")}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["genea140", "cfg3"])
    ap.add_argument("--by", nargs="+", default=["pair", "proband", "ancestor"], choices=["pair", "proband", "ancestor"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--panel", type=int, default=0)
    ap.add_argument("--panels-per-launch", type=int, default=0)
    ap.add_argument("--check-rows", type=int, default=0)
    args = ap.parse_args()
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
