"""gen.phiMatmul / gen.phiSolve on one GPU: genphi_result_matmul and genphi_result_solve on the resident result of a workload, next to
genphi_result_sums on the same matrix in the same run (one read of the matrix) and, once, the host route they replace
(genphi_result_to_host + numpy).  DESIGN.md 19.

    python profiles/phi_matmul_bench.py [--workload cfg3 cfg4] [--reps 5] [--k 1 4 8 16 64] [--ridge 0.5] [--no-host-route]

One JSON line per workload.  Times are host wall clocks in ms around blocking calls (each ends in a stream synchronise), the median
of --reps calls after one warm-up, with [min, max]:
  sums_ms               genphi_result_sums (one pass over the full matrix, 4 N^2 bytes), alternating with the others; sums_gbs
  matmul[k]             matmul_ms = genphi_result_matmul with a standard normal N x k panel in caller arrays: the packing and upload of
                        the panel (8 N k bytes), the kernel, the copy of the product (8 N k bytes) back.  phi_gbs = 4 N^2 bytes
                        x passes / matmul_ms (passes = 1 for k <= 16, ceil(k / 16) beyond: the matrix is read once per tile of 16
                        columns), tflops = 2 N^2 k / matmul_ms, ratio = matmul_ms / sums_ms
  solve                 one genphi_result_solve of 8 standard normal right-hand sides at --ridge, tol = 1e-10: solve_ms, the iteration
                        counts, the largest true residual, ms per product (solve_ms / (max iterations + 1))
  host_route            once: to_host_ms (genphi_result_to_host of the N x N matrix), widen_ms (Float32 -> Float64, 8 N^2 bytes of host
                        memory: skipped above --host-limit probands), numpy_ms (the Float64 product with the k = 8 panel, on as many
                        BLAS threads as the environment sets), max_rel_diff against the device product
Workloads: those of profiles/gc_bench.py (cfg3 = 1e5 individuals / 1e4 probands; cfg4 = the bench pedigree, 1e6 individuals / 1e5
probands: a 40 GB matrix)."""
import argparse
import ctypes as C
import json
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


def run(name, args):
    import genlib_jl_amd as gen
    from gc_bench import load
    ped, pro, _ = load(name)
    L = gen._capi.lib()
    pl = gen.plan(ped, pro)
    try:
        pl.compute_device(device=0)
        n = pl.n_probands
        ks = [k for k in args.k if 1 <= k <= 64]
        res = {"workload": name, "n_pro": n, "reps": args.reps}
        dp = C.POINTER(C.c_double)
        rng = np.random.default_rng(19)
        X = {k: rng.standard_normal((n, k)) for k in ks}
        Y = {k: np.empty((n, k)) for k in ks}

        def matmul(k):
            rc = L.genphi_result_matmul(pl._h, k, X[k].ctypes.data_as(dp), k, Y[k].ctypes.data_as(dp), k, None)
            assert rc == 0, rc

        times = {"sums": []}
        for k in ks:
            times[k] = []
        for rep in range(args.reps + 1):
            row = {"sums": _ms(pl.result_sums)[0]}
            for k in ks:
                row[k] = _ms(lambda: matmul(k))[0]
                _ms(pl.result_sums)
            if rep:                                        # (the first round is the warm-up)
                for key in times:
                    times[key].append(row[key])
        res["sums_ms"] = _stat(times["sums"])
        res["sums_gbs"] = round(4.0 * n * n / res["sums_ms"]["median"] / 1e6, 1)
        res["matmul"] = {}
        for k in ks:
            med = float(np.median(times[k]))
            passes = 1 if k <= 16 else (k + 15) // 16
            res["matmul"][str(k)] = {"matmul_ms": _stat(times[k]), "passes": passes, "phi_gbs": round(4.0 * n * n * passes / med / 1e6, 1),
                                     "tflops": round(2.0 * n * n * k / med / 1e9, 2), "ratio": round(med / res["sums_ms"]["median"], 2)}
        B = rng.standard_normal((n, 8))
        pl.solve(B[:, :1], ridge=args.ridge, maxiter=2)                     # warm-up
        solve_ms, (z, resid, its) = _ms(lambda: pl.solve(B, ridge=args.ridge))
        res["solve"] = {"k": 8, "ridge": args.ridge, "tol": 1e-10, "solve_ms": round(solve_ms, 1), "iterations": [int(i) for i in its],
                        "max_residual": float(resid.max()), "ms_per_product": round(solve_ms / (int(its.max()) + 1), 2)}
        if not args.no_host_route and 8 in ks:
            to_host_ms, phi = _ms(pl.result_to_host)
            route = {"k": 8, "to_host_ms": round(to_host_ms, 1)}
            if n <= args.host_limit:
                widen_ms, phi64 = _ms(lambda: phi.astype(np.float64))
                numpy_ms, ref = _ms(lambda: phi64 @ X[8])
                route.update(widen_ms=round(widen_ms, 1), numpy_ms=round(numpy_ms, 1),
                             max_rel_diff=float((np.abs(ref - Y[8]) / (np.abs(phi64) @ np.abs(X[8]))).max()))
            res["host_route"] = route
        print(json.dumps(res), flush=True)
    finally:
        pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["cfg3", "cfg4"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", nargs="+", type=int, default=[1, 4, 8, 16, 64])
    ap.add_argument("--ridge", type=float, default=0.5)
    ap.add_argument("--host-limit", type=int, default=20000)
    ap.add_argument("--no-host-route", action="store_true")
    args = ap.parse_args()
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
