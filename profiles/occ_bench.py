"""gen.occ and gen.rec on one GPU: device time of the sweep, its algorithmic bytes and the effective bandwidth they give.

    python profiles/occ_bench.py [--workload genea140|cfg3|cfg4|cfg4_16 ...] [--what ind total rec] [--rows 32|64]
                                 [--reps 5] [--panel C] [--check-rows N]

One JSON line per workload and quantity (occ IND, occ TOTAL, rec):
    sweep_ms          median over --reps sweeps after one warm-up (HIP events around the sweep, genphi_occ_stats / genphi_rec_stats)
    algorithmic_bytes for each computed row, its source rows read and its row written at the row width per panel column (occ: 8
                      or 4 bytes per column; rec: 8 bytes per 64 columns), plus the 8-byte result entries (IND), totals or counts,
                      plus (rec) one read of every proband row by the count
    effective_gbs     algorithmic_bytes / sweep_ms: an effective rate (panels are sized for the Infinity Cache), not a share of
                      HBM bandwidth
    row_bits, peak_slots, panel_cols, launches (kernel launches per sweep), device_bytes (device memory taken by the handle:
                      hipMemGetInfo before create and after the first compute; blocks kept by the library's cache included)
--rows 64 forces 64-bit slot rows (default: 32-bit rows for sweeps of at most 31 steps).  --panel C sets the panel width
(GENPHI_OCC_PANEL).  --check-rows N compares N sampled proband rows of IND with the exact counts (tests/occ_oracle.py), TOTAL with
the column sums of IND taken on the device, and rec with the exact oracle in full (results of more than 8 GB are not copied).
Workloads: those of profiles/gc_bench.py.
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


def free_bytes():
    """Free device memory by hipMemGetInfo, from the HIP runtime the library itself is linked against."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    if hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed: no usable GPU")
    return free.value


def sweeps(h, reps):
    times = []
    for r in range(reps + 1):
        h.compute(device=0)
        if r:
            times.append(h.stats()["sweep_ms"])
    return times


def report(name, what, n_pro, n_anc, h, times, used):
    st = h.stats()
    ms = float(np.median(times))
    return {"workload": name, "what": what, "n_pro": n_pro, "n_anc": n_anc, "sweep_ms": round(ms, 3),
            "sweep_ms_all": [round(t, 3) for t in times], "algorithmic_bytes": st["algorithmic_bytes"],
            "effective_gbs": round(st["algorithmic_bytes"] / ms / 1e6, 1), "row_bits": st["row_bits"], "peak_slots": st["peak_slots"],
            "panel_cols": st["panel_cols"], "launches": st["launches"], "device_bytes": int(used)}


def run(name, args):
    import genlib_jl_amd as gen
    from gc_bench import load
    ped, pro, anc = load(name)
    arrs = (ped.ind, ped.father, ped.mother, pro, anc)
    rows64 = args.rows == 64
    ind_totals = None
    for what in args.what:
        gen._capi.lib().genphi_release_cached()
        before = free_bytes()
        if what == "rec":
            h = gen.RecPlan(*arrs)
        else:
            h = gen.OccPlan(*arrs, total_only=what == "total", rows64=rows64)
        try:
            h.compute(device=0)
            used = before - free_bytes()
            res = report(name, what, len(pro), len(anc), h, sweeps(h, args.reps), used)
            if args.check_rows:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                from occ_oracle import occ_exact, rec_exact
                if what == "ind" and 8 * len(pro) * len(anc) <= 8 << 30:
                    sample = np.random.default_rng(1).choice(len(pro), min(args.check_rows, len(pro)), replace=False)
                    ref = occ_exact(ped.ind, ped.father, ped.mother, pro, anc, sample=sample)
                    res["checked_rows"] = len(sample)
                    res["rows_equal_exact"] = bool(np.array_equal(h.result_to_host()[sample].T, ref))
                    ind_totals = h.totals()
                elif what == "total" and ind_totals is not None:
                    res["totals_equal_ind_column_sums"] = bool(np.array_equal(h.totals(), ind_totals))
                elif what == "rec" and len(ped.ind) <= 200_000:
                    res["equal_exact"] = bool(np.array_equal(h.result(), rec_exact(ped.ind, ped.father, ped.mother, pro, anc)))
        finally:
            h.close()
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["genea140", "cfg3", "cfg4", "cfg4_16"])
    ap.add_argument("--what", nargs="+", default=["ind", "total", "rec"], choices=["ind", "total", "rec"])
    ap.add_argument("--rows", type=int, default=32, choices=[32, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--panel", type=int, default=0)
    ap.add_argument("--check-rows", type=int, default=0)
    args = ap.parse_args()
    if args.panel:
        os.environ["GENPHI_OCC_PANEL"] = str(args.panel)
        os.environ["GENPHI_ENV_HOOKS"] = "1"           # (read once, when the library loads)
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
