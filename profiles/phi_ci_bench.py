"""gen.phiCI on one GPU: genphi_result_bootstrap on the resident result of a workload and, once, the host route it replaces
(genphi_result_to_host + the numpy route of gen.phiCI(matrix)).  DESIGN.md 17.

    python profiles/phi_ci_bench.py [--workload genea140 cfg3] [--b 5000] [--reps 3] [--panel 0 P ...] [--no-host-route] [--step-limit 300]

One JSON line per workload and panel width (0 = the default rule; each width gets a plan of its own on the same pedigree,
GENPHI_BOOT_PANEL through the plan's tuning; the host route runs once per workload).  One process; every step that uses the GPU
(the sweep, the warm-up, each timed call, the copy of the matrix) runs under --step-limit seconds: a step that overruns ends the
process at once with a traceback (a watchdog thread: it also ends a call that is stuck in the driver), and any exception ends it
too, so nothing is started on the GPU after a failure.  Times are host wall clocks in ms around blocking calls (each ends in a
stream synchronise), the median of --reps calls after one warm-up call of one panel, with [min, max]:
  boot_ms               PhiPlan.bootstrap(b, seed) on the full resident result: counts, product and reduction of every panel, and
                        the copy of 16 b bytes
  tflops                2 N N b / boot_ms: every entry of the matrix meets every resample once (symmetry is not used)
  host_route            once: to_host_ms (genphi_result_to_host of the N x N matrix), phici_ms (gen.phiCI(matrix, b) on the CPUs
                        the process may use), max_rel_diff of thetastar between the two routes
The counts kernel's share of the call is not measured here: the call offers no way to time one of its kernels from outside.
Workloads: those of profiles/gc_bench.py (cfg3: 1e4 probands; cfg4: 1e5 probands, a 40 GB matrix -- run it with --no-host-route).
"""
import argparse
import contextlib
import faulthandler
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

SEED = 20240611


def _ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


@contextlib.contextmanager
def step(limit):
    """A GPU step under its own time limit: the process exits with a traceback if the block takes longer."""
    faulthandler.dump_traceback_later(limit, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _stat(times):
    return {"median": round(float(np.median(times)), 3), "min": round(min(times), 3), "max": round(max(times), 3)}


def run(name, args):
    from gc_bench import load
    ped, pro, _ = load(name)
    host_route = not args.no_host_route
    for panel in args.panel:
        run_one(name, ped, pro, panel, host_route, args)
        host_route = False


def run_one(name, ped, pro, panel, host_route, args):
    import genlib_jl_amd as gen
    tuning = {}
    if panel:
        tuning["BOOT_PANEL"] = panel
    pl = gen.plan(ped, pro, tuning=tuning)
    try:
        with step(args.step_limit):
            pl.compute_device(device=0)
        n, b = pl.n_probands, args.b
        res = {"workload": name, "n_pro": n, "b": b, "reps": args.reps, "panel": panel or "default"}
        with step(args.step_limit):
            pl.bootstrap(min(b, 128), SEED)                                    # warm-up: one panel
        times, out = [], None
        for _ in range(args.reps):
            with step(args.step_limit):
                t, out = _ms(lambda: pl.bootstrap(b, SEED))
            times.append(t)
        res["boot_ms"] = _stat(times)
        res["tflops"] = round(2.0 * n * n * b / res["boot_ms"]["median"] / 1e9, 2)
        theta = (out[0] - out[1]) / (float(n) * (n - 1))
        res["theta_quantiles"] = [float(q) for q in np.quantile(theta, [0.025, 0.975])]
        if host_route:
            with step(args.step_limit):
                to_host_ms, phi = _ms(pl.result_to_host)
            phici_ms, host = _ms(lambda: gen.phiCI(phi, b=b, seed=SEED))
            res["host_route"] = {"to_host_ms": round(to_host_ms, 1), "phici_ms": round(phici_ms, 1),
                                 "max_rel_diff": float(np.max(np.abs(host.thetastar - theta) / host.thetastar))}
            del phi
        print(json.dumps(res), flush=True)
    finally:
        pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["genea140", "cfg3"])
    ap.add_argument("--b", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--panel", type=int, nargs="+", default=[0])
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--step-limit", type=int, default=300, help="seconds a single GPU step may take")
    args = ap.parse_args()
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
