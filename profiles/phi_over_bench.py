"""gen.phiOver on one GPU: genphi_result_over on the resident result of a workload, next to genphi_result_sums on the same matrix
and, once, the host route it replaces (genphi_result_to_host + numpy).  DESIGN.md 16.

    python profiles/phi_over_bench.py [--workload cfg4] [--reps 5] [--targets 1e3 1e6 1e8] [--no-host-route]

One JSON line per workload.  Times are host wall clocks in ms around blocking calls (each ends in a stream synchronise), the
median of --reps calls after one warm-up, with [min, max]:
  count_ms              the count-only call (one pass over the upper triangle) at the 1e6 threshold, the kept counts dropped before
                        each call; count_gbs = 2 N^2 bytes / count_ms
  sums_ms               genphi_result_sums (one pass over the full matrix, 4 N^2 bytes), alternating with the others; sums_gbs
  fill[target]          per target number of pairs: the threshold found by bisection on count-only calls (Float32 values, so that
                        the numpy comparison of the host route is the same test), pairs = what it selects, fill_ms = the filling
                        call with no counts kept (count + write + copy), fill_kept_ms = the filling call right after a count-only
                        call of the same threshold (write + copy), phi_over_ms = PhiPlan.phi_over (count, allocate, fill)
  host_route            once: to_host_ms (genphi_result_to_host of the N x N matrix), select_ms (numpy on its strict upper triangle,
                        in row blocks, at the 1e6 threshold), equal = the lists are the same
Workloads: those of profiles/gc_bench.py (cfg4 = the bench pedigree, 1e6 individuals / 1e5 probands: a 40 GB matrix).
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)


def _ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def _stat(times):
    return {"median": round(float(np.median(times)), 3), "min": round(min(times), 3), "max": round(max(times), 3)}


def threshold_for(pl, target):
    """The largest Float32 threshold in (0, 1] that selects at least `target` pairs (bisection on the bit patterns of the
    positive floats, which order like the values), and the number it selects."""
    lo, hi = int(np.float32(2.0 ** -100).view(np.int32)), int(np.float32(1.0).view(np.int32))
    as_t = lambda bits: float(np.int32(bits).view(np.float32))  # noqa: E731
    if pl.count_over(as_t(lo)) < target:
        return as_t(lo), pl.count_over(as_t(lo))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pl.count_over(as_t(mid)) >= target:
            lo = mid
        else:
            hi = mid
    return as_t(lo), pl.count_over(as_t(lo))


def host_select(phi, t, block=2048):
    """The parent commit's route: numpy on the strict upper triangle of the host matrix, by row blocks."""
    t32 = np.float32(t)
    assert float(t32) == t
    rows, cols, vals = [], [], []
    for a in range(0, len(phi), block):
        blk = phi[a:a + block]
        hit = blk >= t32
        hit &= np.arange(phi.shape[1])[None, :] > (a + np.arange(len(blk)))[:, None]
        k, j = np.nonzero(hit)
        rows.append((k + a).astype(np.int32)); cols.append(j.astype(np.int32)); vals.append(blk[k, j])
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)


def run(name, args):
    import genlib_jl_amd as gen
    from gc_bench import load
    ped, pro, _ = load(name)
    L = gen._capi.lib()
    pl = gen.plan(ped, pro)
    try:
        pl.compute_device(device=0)
        n = pl.n_probands
        res = {"workload": name, "n_pro": n, "pairs": n * (n - 1) // 2, "reps": args.reps}
        picks = {("%g" % tg): threshold_for(pl, int(tg)) for tg in args.targets}
        t_mid = picks["%g" % args.targets[len(args.targets) // 2]][0]
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        bufs = {k: (np.empty(m, np.int32), np.empty(m, np.int32), np.empty(m, np.float32)) for k, (_, m) in picks.items()}

        def drop_counts():
            pl.count_over(math.inf)                       # another threshold: the kept counts are replaced

        def fill(key):
            t, m = picks[key]
            r, c, v = bufs[key]
            got = C.c_int64()
            rc = L.genphi_result_over(pl._h, t, m, r.ctypes.data_as(i32p), c.ctypes.data_as(i32p), v.ctypes.data_as(f32p), C.byref(got))
            assert rc == 0 and got.value == m, (rc, got.value, m)

        times = {"count": [], "sums": []}
        for key in picks:
            times["fill " + key], times["kept " + key], times["phi_over " + key] = [], [], []
        for rep in range(args.reps + 1):
            row = {}
            drop_counts()
            row["count"] = _ms(lambda: pl.count_over(t_mid))[0]
            row["sums"] = _ms(pl.result_sums)[0]
            for key in picks:
                drop_counts()
                row["fill " + key] = _ms(lambda: fill(key))[0]
                row["sums2"] = _ms(pl.result_sums)[0]
                drop_counts()
                pl.count_over(picks[key][0])
                row["kept " + key] = _ms(lambda: fill(key))[0]
                drop_counts()
                row["phi_over " + key] = _ms(lambda: pl.phi_over(picks[key][0]))[0]
            if rep:                                        # (the first round is the warm-up)
                for k in times:
                    times[k].append(row[k])
        res["count_ms"], res["sums_ms"] = _stat(times["count"]), _stat(times["sums"])
        res["count_gbs"] = round(2.0 * n * n / res["count_ms"]["median"] / 1e6, 1)
        res["sums_gbs"] = round(4.0 * n * n / res["sums_ms"]["median"] / 1e6, 1)
        res["fill"] = {key: {"threshold": picks[key][0], "pairs": picks[key][1], "fill_ms": _stat(times["fill " + key]),
                             "fill_kept_ms": _stat(times["kept " + key]), "phi_over_ms": _stat(times["phi_over " + key])} for key in picks}
        if not args.no_host_route:
            key = "%g" % args.targets[len(args.targets) // 2]
            fill(key)
            to_host_ms, phi = _ms(pl.result_to_host)
            select_ms, ref = _ms(lambda: host_select(phi, picks[key][0]))
            res["host_route"] = {"threshold": picks[key][0], "to_host_ms": round(to_host_ms, 1), "select_ms": round(select_ms, 1),
                                 "equal": bool(all(np.array_equal(a, b) for a, b in zip(ref, bufs[key])))}
        print(json.dumps(res), flush=True)
    finally:
        pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["cfg4"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--targets", nargs="+", type=float, default=[1e3, 1e6, 1e8])
    ap.add_argument("--no-host-route", action="store_true")
    args = ap.parse_args()
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
