"""gen.phiClusters / gen.phiUnrelated on one GPU: genphi_result_clusters and genphi_result_unrelated on the resident result of a
workload, next to the count-only genphi_result_over (the same walk of the upper triangle with no union) and genphi_result_sums (one
read of the whole matrix) on the same matrix.  DESIGN.md 26.

    python profiles/phi_clusters_bench.py [--workload synth2500 cfg4] [--reps 5] [--thresholds 0.125 0.015625 0.0009765625 0]

One JSON line per workload.  Times are host wall clocks in ms around blocking calls (each ends in a stream synchronise), the median
of --reps calls after one warm-up, with [min, max]; per threshold:
  pairs, clusters, largest, kept, rounds     what the queries answer (rounds: the launches of the round kernel, by degree)
  count_ms              the count-only genphi_result_over, the kept counts dropped before each call: 2 N^2 bytes
  clusters_ms           genphi_result_clusters with the labels: 2 N^2 bytes + a pass over N entries + 4 N bytes back
  degree_rounds_ms      genphi_result_unrelated without priorities: the degree pass (4 N^2 bytes) + the rounds
  rounds_only_ms        genphi_result_unrelated with equal priorities and no degrees asked for: the rounds alone; rounds_position
  *_share               the bytes of the model (2 N^2, 2 N^2, 4 N^2) / the time, over the copy rate COPY_TBS
and once sums_ms (4 N^2 bytes).  Kernel times apart from the host clock come from running this script under
`rocprofv3 --kernel-trace --stats -- python profiles/phi_clusters_bench.py ...` (cluster_union_kernel, cluster_flatten_kernel,
degree_kernel, unrelated_round_kernel, over_count_kernel, row_sums_kernel in the statistics).
Workloads: synth2500 = the 2,500 probands of tests/test_phi_clusters_gpu.py; the others are those of profiles/gc_bench.py (cfg3: 1e4
probands; cfg4: 1e5 probands, a 40 GB matrix).
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

COPY_TBS = 6.29          # the float4 copy rate of an MI355X (of 8.0 TB/s peak)


def _ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def _stat(times):
    return {"median": round(float(np.median(times)), 3), "min": round(min(times), 3), "max": round(max(times), 3)}


def load(name):
    import genlib_jl_amd as gen
    if name == "synth2500":
        from genlib_jl_amd import synth
        ind, fa, mo, sex, pro = synth.random_mating(30_000, 2_500, 10, skip_permille=50)
        return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}), pro
    from gc_bench import load as load_gc
    ped, pro, _ = load_gc(name)
    return ped, pro


def run(name, args):
    import genlib_jl_amd as gen
    ped, pro = load(name)
    L = gen._capi.lib()
    pl = gen.plan(ped, pro)
    try:
        pl.compute_device(device=0)
        n = pl.n_probands
        res = {"workload": name, "n_pro": n, "reps": args.reps, "copy_tbs": COPY_TBS}
        i32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        label, member, zeros = np.empty(n, np.int32), np.empty(n, np.uint8), np.zeros(n, np.int32)
        share = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / (COPY_TBS * 1e12), 3)  # noqa: E731

        def clusters(t):
            k, pairs = C.c_int64(), C.c_int64()
            rc = L.genphi_result_clusters(pl._h, t, label.ctypes.data_as(i32p), C.byref(k), C.byref(pairs))
            assert rc == 0, gen._capi.last_error()
            return k.value, pairs.value

        def rounds_only(t):
            rounds = C.c_int32()
            rc = L.genphi_result_unrelated(pl._h, t, zeros.ctypes.data_as(i32p), member.ctypes.data_as(u8p), None, None, C.byref(rounds))
            assert rc == 0, gen._capi.last_error()
            return rounds.value

        sums = []
        per_t = {}
        for t in args.thresholds:
            times = {"count": [], "clusters": [], "degree_rounds": [], "rounds_only": []}
            for rep in range(args.reps + 1):
                row = {}
                pl.count_over(math.inf)                      # another threshold: the kept counts are replaced
                row["count"], pairs = _ms(lambda: pl.count_over(t))
                s_ms = _ms(pl.result_sums)[0]
                row["clusters"], (k, pairs2) = _ms(lambda: clusters(t))
                assert pairs == pairs2
                largest = int(np.bincount(label).max())
                row["degree_rounds"], (keep, degree, rounds) = _ms(lambda: pl.unrelated(t))
                row["rounds_only"], rounds_position = _ms(lambda: rounds_only(t))
                if rep:                                      # (the first round is the warm-up)
                    sums.append(s_ms)
                    for key in times:
                        times[key].append(row[key])
            st = {key + "_ms": _stat(v) for key, v in times.items()}
            st.update(threshold=t, pairs=pairs, clusters=k, largest=largest, kept=int(keep.sum()), rounds=rounds, rounds_position=rounds_position,
                      count_share=share(2.0 * n * n, st["count_ms"]["median"]), clusters_share=share(2.0 * n * n, st["clusters_ms"]["median"]),
                      degree_rounds_share=share(4.0 * n * n, st["degree_rounds_ms"]["median"]))
            per_t["%g" % t] = st
        res["sums_ms"] = _stat(sums)
        res["sums_share"] = share(4.0 * n * n, res["sums_ms"]["median"])
        res["thresholds"] = per_t
        print(json.dumps(res), flush=True)
    finally:
        pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["synth2500", "cfg4"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--thresholds", nargs="+", type=float, default=[1 / 8, 1 / 64, 1 / 1024, 0.0])
    args = ap.parse_args()
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
