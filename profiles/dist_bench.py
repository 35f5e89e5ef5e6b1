"""gen.meioses and gen.findMRCA on one GPU: device time of the sweep, its algorithmic bytes and the effective bandwidth they give.

    python profiles/dist_bench.py [--workload genea140|cfg3|cfg4|cfg4_16 ...] [--reps 5] [--panel C] [--check-rows N]
                                  [--mrca N [N ...]]

One JSON line per workload (what = "meioses"), in the form of profiles/occ_bench.py (run both back to back to compare: the
yardstick is occ IND with 32-bit rows on the same workload):
    sweep_ms          median over --reps sweeps after one warm-up (HIP events around the sweep, genphi_dist_stats)
    algorithmic_bytes for each computed row, its source rows read and its row written at 2 bytes per panel column, plus the
                      2-byte result entries
    effective_gbs     algorithmic_bytes / sweep_ms: an effective rate (panels are sized for the Infinity Cache), not a share of
                      HBM bandwidth
    row_bits, peak_slots, panel_cols, launches (kernel launches per sweep), device_bytes (device memory taken by the handle:
                      hipMemGetInfo before create and after the first compute; blocks kept by the library's cache included)
--panel C sets the panel width (GENPHI_DIST_PANEL).  --check-rows N compares N sampled proband rows with the breadth-first search
of tests/mrca_oracle.py.  --mrca N ...: one more JSON line per N (what = "findMRCA") for the first N probands of the workload: the
wall time of gen.findMRCA (median of --reps calls after a warm-up) split into its parts -- ancestors (host), rec (GPU call, its
planning included), filter (host), sweep (the gen.meioses call, planning and copy included) -- and the counts of common ancestors
and MRCAs.  Workloads: those of profiles/gc_bench.py.
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

from occ_bench import free_bytes, report, sweeps  # noqa: E402


def mrca_parts(gen, ped, ids):
    """findMRCA step by step (the steps of genlib_jl_amd.findMRCA), each timed on the host clock."""
    t = [time.perf_counter()]
    distinct = np.unique(ids)
    candidates = min((gen.ancestor(ped, [i]) for i in distinct[:gen._MRCA_CANDIDATE_SEARCHES]), key=len)
    t.append(time.perf_counter())
    common = candidates[gen.rec(ped, distinct, candidates, device=0) == len(distinct)] if len(candidates) else candidates
    t.append(time.perf_counter())
    mrcas = gen._capi.mrca_filter(ped.ind, ped.father, ped.mother, common)
    t.append(time.perf_counter())
    m = gen.meioses(ped, ids, mrcas, device=0) if len(mrcas) else np.zeros((len(ids), 0), dtype=np.int16)
    t.append(time.perf_counter())
    return np.diff(t) * 1e3, len(common), len(mrcas), m


def run(name, args):
    import genlib_jl_amd as gen
    from gc_bench import load
    ped, pro, anc = load(name)
    gen._capi.lib().genphi_release_cached()
    before = free_bytes()
    h = gen.DistPlan(ped.ind, ped.father, ped.mother, pro, anc)
    try:
        h.compute(device=0)
        used = before - free_bytes()
        res = report(name, "meioses", len(pro), len(anc), h, sweeps(h, args.reps), used)
        if args.check_rows:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from mrca_oracle import meioses_exact
            sample = np.random.default_rng(1).choice(len(pro), min(args.check_rows, len(pro)), replace=False)
            ref = meioses_exact(ped.ind, ped.father, ped.mother, pro, anc, sample=sample)
            res["checked_rows"] = len(sample)
            res["rows_equal_exact"] = bool(np.array_equal(h.result_to_host()[sample], ref))
    finally:
        h.close()
    print(json.dumps(res), flush=True)
    for n in args.mrca:
        ids = pro[:n]
        parts, walls = [], []
        for r in range(args.reps + 1):
            p, n_common, n_mrca, m = mrca_parts(gen, ped, ids)
            t0 = time.perf_counter()
            whole = gen.findMRCA(ped, ids, device=0)
            wall = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(whole.meioses, m)
            if r:
                parts.append(p)
                walls.append(wall)
        med = np.median(np.array(parts), axis=0)
        print(json.dumps({"workload": name, "what": "findMRCA", "n_ids": int(n), "common": n_common, "mrcas": n_mrca,
                          "wall_ms": round(float(np.median(walls)), 3), "wall_ms_all": [round(w, 3) for w in walls],
                          "ancestors_ms": round(float(med[0]), 3), "rec_ms": round(float(med[1]), 3),
                          "filter_ms": round(float(med[2]), 3), "sweep_ms": round(float(med[3]), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["genea140", "cfg3", "cfg4"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--panel", type=int, default=0)
    ap.add_argument("--check-rows", type=int, default=0)
    ap.add_argument("--mrca", type=int, nargs="*", default=[])
    args = ap.parse_args()
    if args.panel:
        os.environ["GENPHI_DIST_PANEL"] = str(args.panel)
        os.environ["GENPHI_ENV_HOOKS"] = "1"           # (read once, when the library loads)
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
