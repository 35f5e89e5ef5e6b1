"""gen.phiEigen on one GPU: genphi_result_eigen on the resident result of a workload, next to a one-column genphi_result_matmul call and
genphi_result_sums on the same matrix in the same run, alternating, and, once, the host route it replaces (genphi_result_to_host +
numpy.linalg.eigvalsh).  DESIGN.md 21.

    python profiles/phi_eigen_bench.py [--workload cfg3 cfg4] [--reps 5] [--k 1 4 10] [--tol 1e-8] [--no-host-route]

One JSON line per workload.  Times are host wall clocks in ms around blocking calls, the median of --reps calls after one warm-up,
with [min, max]:
  sums_ms, matmul1_ms   genphi_result_sums (one read of the matrix) and genphi_result_matmul with one standard normal column in caller
                        arrays (packing, upload, kernel, download), alternating with the eigen calls
  eigen[k][plain|centred]  eigen_ms = one genphi_result_eigen call (k pairs, tol, maxiter 300, seed 0: the scratch request, the clearing
                        of the block, every Lanczos step, the eigenvectors of T, the Ritz vectors, the residual product, the download);
                        products, converged (how many of k), max_residual, ms_per_product = eigen_ms / products, and
                        ratio_to_matmul1 = ms_per_product / matmul1_ms: the traffic model says <= 1 once the matrix read
                        dominates
  host_route            once, up to --host-limit probands: to_host_ms, eigvalsh_ms (Float64 numpy.linalg.eigvalsh of the whole matrix: values
                        only, eigh with vectors costs more),
                        max_value_diff against the device's k = 10 plain values
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
        res = {"workload": name, "n_pro": n, "reps": args.reps, "tol": args.tol}
        dp = C.POINTER(C.c_double)
        x, y = np.random.default_rng(21).standard_normal((n, 1)), np.empty((n, 1))

        def matmul1():
            rc = L.genphi_result_matmul(pl._h, 1, x.ctypes.data_as(dp), 1, y.ctypes.data_as(dp), 1, None)
            assert rc == 0, rc

        forms = [(k, c) for k in args.k for c in (False, True)]
        times = {"sums": [], "matmul1": []}
        last = {}
        for f in forms:
            times[f] = []
        for rep in range(args.reps + 1):
            row = {}
            for f in forms:
                row.setdefault("sums", _ms(pl.result_sums)[0])
                row.setdefault("matmul1", _ms(matmul1)[0])
                row[f], last[f] = _ms(lambda: pl.eigen(f[0], f[1], args.tol))
                _ms(pl.result_sums)
                _ms(matmul1)
            if rep:                                        # (the first round is the warm-up)
                for key in times:
                    times[key].append(row[key])
        res["sums_ms"] = _stat(times["sums"])
        res["matmul1_ms"] = _stat(times["matmul1"])
        res["eigen"] = {}
        for k, c in forms:
            val, vec, resid, conv, m = last[(k, c)]
            med = float(np.median(times[(k, c)]))
            res["eigen"].setdefault(str(k), {})["centred" if c else "plain"] = {
                "eigen_ms": _stat(times[(k, c)]), "products": m, "converged": int(conv.sum()), "max_residual": float(resid.max()),
                "ms_per_product": round(med / m, 4), "ratio_to_matmul1": round(med / m / res["matmul1_ms"]["median"], 3)}
        if not args.no_host_route and n <= args.host_limit and (10, False) in last:
            to_host_ms, phi = _ms(pl.result_to_host)
            eigvalsh_ms, lam = _ms(lambda: np.linalg.eigvalsh(phi.astype(np.float64)))
            res["host_route"] = {"to_host_ms": round(to_host_ms, 1), "eigvalsh_ms": round(eigvalsh_ms, 1),
                                 "max_value_diff": float(np.abs(lam[::-1][:10] - last[(10, False)][0]).max())}
        print(json.dumps(res), flush=True)
    finally:
        pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["cfg3", "cfg4"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", nargs="+", type=int, default=[1, 4, 10])
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--host-limit", type=int, default=20000)
    ap.add_argument("--no-host-route", action="store_true")
    args = ap.parse_args()
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
