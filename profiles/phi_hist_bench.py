"""gen.phiHist / gen.phiQuantile on one GPU: genphi_result_hist and genphi_result_select on the resident result of a workload, next to
the two queries that read the same bytes (the counting pass of genphi_result_over: the floor; genphi_result_sums) and, at N = 1e4
only, the host route they replace (genphi_result_to_host + np.histogram / np.partition).  DESIGN.md 20.

    python profiles/phi_hist_bench.py [--workload cfg3 cfg4 zeros] [--reps 5] [--no-host-route] [--lib PATH]
    python profiles/phi_hist_bench.py --build-variants          # build/hist_ab/libgenphi_{agg0,agg2,agg64,entry2}.so
    python profiles/phi_hist_bench.py --ab [--workload ...]      # every variant built, two rounds, one process per (round, variant)

One JSON line per workload.  Times are host wall clocks in ms around blocking calls (each ends in a stream synchronise), the median
of --reps calls after one warm-up, with [min, max]; the calls of one repetition alternate, so a drift of the clock meets all of them:
  count_over_ms         the count-only call of genphi_result_over at threshold 0.0 (one pass over the upper triangle, the kept counts
                        dropped before each call); sums_ms: genphi_result_sums (the full matrix)
  hist64_ms, hist4096_ms   64 and 4,096 uniform bins over [0, 0.5], no labels; hist64_g7_ms: 64 bins, 7 groups that are runs of the proband order;
                        hist64_g7_mixed_ms: the same with labels k % 7
  select1_ms, select16_ms  the median alone; 16 ranks spread over the pairs
  ratio_hist64          hist64_ms / count_over_ms (medians)
  zero_share            the share of pairs that are exactly zero (from a histogram)
  host_route            N <= 10,000 only: to_host_ms, histogram_ms (np.histogram, 64 bins, of the strict upper triangle),
                        partition_ms (np.partition at the median), equal = both agree with the device; otherwise "not run"
Workloads: cfg3 (1e5 individuals, 1e4 probands, 20 generations), cfg4 (the bench pedigree: 1e6 individuals, 1e5 probands, 30
generations: a 40 GB matrix) and zeros (4e5 individuals, 2e4 probands, 4 generations: as in genea140 most pairs are unrelated).
--lib PATH loads that build of the library instead of genlib.jl_amd/lib/libgenphi.so (a variant of --build-variants); the form of
the LDS update is a compile-time choice of csrc/hist.hip, so an A/B is a run per library."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
AB_DIR = os.path.join(ROOT, "build", "hist_ab")
VARIANTS = ("agg0", "agg2", "agg64", "entry2")     # rounds of wave aggregation before the plain LDS atomic (0: one atomic per entry);
DEFINES = {"agg0": ["-DGENPHI_HIST_AGG_ROUNDS=0"], "agg2": ["-DGENPHI_HIST_AGG_ROUNDS=2"], "agg64": ["-DGENPHI_HIST_AGG_ROUNDS=64"],
           "entry2": ["-DGENPHI_HIST_AGG_ROUNDS=2", "-DGENPHI_HIST_ENTRYWISE=1"]}     # entry2: two rounds, one entry of a lane at a time


def _ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def _stat(times):
    return {"median": round(float(np.median(times)), 3), "min": round(min(times), 3), "max": round(max(times), 3)}


def load(name):
    import genlib_jl_amd as gen
    from genlib_jl_amd import synth
    shape = {"cfg3": (100_000, 10_000, 20), "cfg4": (1_000_000, 100_000, 30), "zeros": (400_000, 20_000, 4)}[name]
    ind, fa, mo, sex, pro = synth.random_mating(*shape)
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}), pro


def run(name, args):
    import genlib_jl_amd as gen
    ped, pro = load(name)
    pl = gen.plan(ped, pro)
    try:
        pl.compute_device(device=0)
        n = pl.n_probands
        pairs = pl.count_pairs()
        res = {"workload": name, "lib": os.path.basename(gen._capi.LIB_PATH), "n_pro": n, "pairs": pairs, "reps": args.reps}
        e64, e4096 = np.linspace(0.0, 0.5, 65), np.linspace(0.0, 0.5, 4097)
        labels = (np.arange(n) * 7 // n).astype(np.int32)        # 7 runs, as gen.phiHist orders the probands; and interleaved
        mixed = (np.arange(n) % 7).astype(np.int32)
        r16 = (np.arange(16) * (pairs // 16) + pairs // 32).astype(np.int64)
        calls = {"count_over": None, "sums": pl.result_sums,
                 "hist64": lambda: pl.hist(e64), "hist4096": lambda: pl.hist(e4096), "hist64_g7": lambda: pl.hist(e64, labels, 7),
                 "hist64_g7_mixed": lambda: pl.hist(e64, mixed, 7),
                 "select1": lambda: pl.select([pairs // 2]), "select16": lambda: pl.select(r16)}
        if args.only_hist:
            calls = {k: v for k, v in calls.items() if not k.startswith("select") and k != "sums"}
        times = {k: [] for k in calls}
        for rep in range(args.reps + 1):
            for k, fn in calls.items():
                if k == "count_over":
                    pl.count_over(math.inf)                # (another threshold: the kept counts are replaced; timed alone below)
                    t = _ms(lambda: pl.count_over(0.0))[0]
                else:
                    t = _ms(fn)[0]
                if rep:                                    # (the first round is the warm-up)
                    times[k].append(t)
        for k in calls:
            res[k + "_ms"] = _stat(times[k])
        res["ratio_hist64"] = round(res["hist64_ms"]["median"] / res["count_over_ms"]["median"], 2)
        res["count_over_gbs"] = round(2.0 * n * n / res["count_over_ms"]["median"] / 1e6, 1)
        res["hist64_gbs"] = round(2.0 * n * n / res["hist64_ms"]["median"] / 1e6, 1)
        tiny = float(np.nextafter(np.float64(0.0), 1.0))
        res["zero_share"] = round(int(pl.hist([0.0, tiny, 1.0])[0][0]) / max(pairs, 1), 4)
        if args.no_host_route or args.only_hist or n > 10_000:
            res["host_route"] = "not run"
        else:
            counts, median = pl.hist(e64)[0], pl.select([pairs // 2])[0]
            to_host_ms, phi = _ms(pl.result_to_host)
            hist_ms, ref = _ms(lambda: np.histogram(phi[np.triu_indices(n, 1)].astype(np.float64), bins=e64)[0])
            part_ms, ref_med = _ms(lambda: np.partition(phi[np.triu_indices(n, 1)], pairs // 2)[pairs // 2])
            res["host_route"] = {"to_host_ms": round(to_host_ms, 1), "histogram_ms": round(hist_ms, 1), "partition_ms": round(part_ms, 1),
                                 "equal": bool(np.array_equal(ref, counts) and ref_med == median)}
        print(json.dumps(res), flush=True)
    finally:
        pl.close()


def build_variants():
    """csrc/hist.hip once per value of GENPHI_HIST_AGG_ROUNDS, linked with the objects build() left in build/obj."""
    import __graft_entry__ as G
    G.build()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(ROOT, "build", "obj")
    os.makedirs(AB_DIR, exist_ok=True)
    others = sorted(os.path.join(objdir, f) for f in os.listdir(objdir) if f.endswith(".o") and f != "hist.hip.o")
    cflags = [f for f in G.HIPCC_FLAGS if f != "-shared"]
    for k in VARIANTS:
        obj = os.path.join(AB_DIR, "hist_%s.o" % k)
        subprocess.check_call([hipcc] + cflags + DEFINES[k] + ["-c", os.path.join(G.PKG, "csrc", "hist.hip"), "-o", obj])
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + others + [obj, "-o", os.path.join(AB_DIR, "libgenphi_%s.so" % k)])
        print("built", os.path.join(AB_DIR, "libgenphi_%s.so" % k), flush=True)


def ab(args):
    libs = [os.path.join(AB_DIR, "libgenphi_%s.so" % k) for k in VARIANTS]
    libs = [p for p in libs if os.path.exists(p)]
    if len(libs) < 2:
        sys.exit("no variants under %s: run --build-variants where the sources compile" % AB_DIR)
    for rnd in range(2):
        for lib in libs:
            cmd = [sys.executable, os.path.abspath(__file__), "--lib", lib, "--only-hist", "--reps", str(args.reps), "--workload"] + args.workload
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
            if rc != 0:                                    # nothing more is started on the GPU after a failure
                sys.exit("round %d, %s: exit status %d" % (rnd, lib, rc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["cfg3", "cfg4"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--only-hist", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--timeout", type=float, default=280.0, help="seconds one process of --ab may take")
    args = ap.parse_args()
    if args.build_variants:
        return build_variants()
    if args.ab:
        return ab(args)
    if args.lib:
        from genlib_jl_amd import _capi
        _capi.LIB_PATH = os.path.abspath(args.lib)
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
