"""gen.phiNearest on one GPU: genphi_result_nearest on the resident result of a workload, next to genphi_result_sums on the same
matrix in the same run and, once, the host route it replaces (genphi_result_to_host + numpy argpartition).  DESIGN.md 18.

    python profiles/phi_nearest_bench.py [--workload genea140 cfg3 cfg4] [--reps 5] [--k 1 10 64] [--buf B] [--no-host-route]

One JSON line per workload.  Times are host wall clocks in ms around blocking calls (each ends in a stream synchronise), the
median of --reps calls after one warm-up, with [min, max]:
  sums_ms               genphi_result_sums (one pass over the full matrix, 4 N^2 bytes), alternating with the others; sums_gbs
  nearest[k]            nearest_ms = genphi_result_nearest into caller arrays (one pass over the full matrix, the copy of the
                        8 N k bytes of output included), nearest_gbs = 4 N^2 bytes / nearest_ms, ratio = nearest_ms / sums_ms
  host_route            once, at the middle k: to_host_ms (genphi_result_to_host of the N x N matrix), select_ms (per row
                        argpartition of the k largest off-diagonal values and a sort of those k, row blocks on --threads threads),
                        values_equal = the kinships are those of the device (the columns may differ where values tie at the cut:
                        argpartition does not order ties)
Workloads: those of profiles/gc_bench.py (cfg3 = 1e5 individuals / 1e4 probands; cfg4 = the bench pedigree, 1e6 individuals /
1e5 probands: a 40 GB matrix).  --buf sets GENPHI_NEAREST_BUF for the plan (the result does not depend on it).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

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


def host_select(phi, k, threads, block=512):
    """The route without genphi_result_nearest: numpy on the host matrix, by row blocks on a thread pool.  Returns the k largest
    off-diagonal values of every row, largest first."""
    n = len(phi)
    out = np.empty((n, k), dtype=np.float32)

    def work(a):
        blk = phi[a:a + block].copy()
        blk[np.arange(len(blk)), a + np.arange(len(blk))] = -1.0            # the diagonal is no candidate
        top = np.argpartition(blk, n - k, axis=1)[:, n - k:]
        out[a:a + block] = -np.sort(-np.take_along_axis(blk, top, axis=1), axis=1)

    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(work, range(0, n, block)))
    return out


def run(name, args):
    import genlib_jl_amd as gen
    from gc_bench import load
    ped, pro, _ = load(name)
    L = gen._capi.lib()
    pl = gen.plan(ped, pro, tuning={} if not args.buf else {"NEAREST_BUF": args.buf})
    try:
        pl.compute_device(device=0)
        n = pl.n_probands
        ks = [k for k in args.k if k <= min(n - 1, 64)]
        res = {"workload": name, "n_pro": n, "reps": args.reps, "nearest_buf": int(pl.stats.nearest_buf)}
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        bufs = {k: (np.empty((n, k), np.int32), np.empty((n, k), np.float32)) for k in ks}

        def nearest(k):
            c, v = bufs[k]
            rc = L.genphi_result_nearest(pl._h, k, c.ctypes.data_as(i32p), v.ctypes.data_as(f32p))
            assert rc == 0, rc

        times = {"sums": []}
        for k in ks:
            times[k] = []
        for rep in range(args.reps + 1):
            row = {"sums": _ms(pl.result_sums)[0]}
            for k in ks:
                row[k] = _ms(lambda: nearest(k))[0]
                _ms(pl.result_sums)
            if rep:                                        # (the first round is the warm-up)
                for key in times:
                    times[key].append(row[key])
        res["sums_ms"] = _stat(times["sums"])
        res["sums_gbs"] = round(4.0 * n * n / res["sums_ms"]["median"] / 1e6, 1)
        res["nearest"] = {str(k): {"nearest_ms": _stat(times[k]), "nearest_gbs": round(4.0 * n * n / np.median(times[k]) / 1e6, 1),
                                   "ratio": round(float(np.median(times[k])) / res["sums_ms"]["median"], 2)} for k in ks}
        if not args.no_host_route and ks:
            k = ks[len(ks) // 2]
            to_host_ms, phi = _ms(pl.result_to_host)
            select_ms, ref = _ms(lambda: host_select(phi, k, args.threads))
            res["host_route"] = {"k": k, "threads": args.threads, "to_host_ms": round(to_host_ms, 1), "select_ms": round(select_ms, 1),
                                 "values_equal": bool(np.array_equal(ref, bufs[k][1]))}
        print(json.dumps(res), flush=True)
    finally:
        pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["genea140", "cfg3", "cfg4"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", nargs="+", type=int, default=[1, 10, 64])
    ap.add_argument("--buf", type=int, default=0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-host-route", action="store_true")
    args = ap.parse_args()
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
