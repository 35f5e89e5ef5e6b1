"""gen.phiTree on one GPU: genphi_result_tree on the resident result of a workload, next to genphi_result_sums (one read of the whole
matrix: the most a round reads) and genphi_result_clusters at the same threshold (one read of the upper triangle) on the same matrix.
DESIGN.md 29.

    python profiles/phi_tree_bench.py [--workload cfg3 cfg4] [--reps 5] [--floors none 0.0009765625 0.015625 0.125]

One JSON line per workload.  Times are host wall clocks in ms around blocking calls (each ends in a stream synchronise), the median
of --reps calls after one warm-up, with [min, max]; per floor ("none": the smallest positive Float32):
  edges, trees, rounds  what the query answers
  tree_ms               genphi_result_tree with its three arrays: the rounds, N - 1 records back, the host's sort
  per_round_ms          tree_ms / rounds
  round_over_sums       per_round_ms / sums_ms: the expectation is <= about 1 (a round reads at most the matrix once)
  clusters_ms           genphi_result_clusters at the floor, with the labels
  active_share          per round, the share of the rows that were read: those of components still growing when the round began.
                        Replayed on the host from the N - 1 edges returned: Boruvka's rounds on the forest alone pick what they
                        pick on the whole graph, since every pick is an edge of the forest.
and once sums_ms (4 N^2 bytes) with sums_share, its bytes over the time over the copy rate COPY_TBS.  Kernel times apart from the
host clock come from running this script under `rocprofv3 --kernel-trace --stats -- python profiles/phi_tree_bench.py ...`
(tree_row_kernel, tree_level_kernel, tree_pick_kernel, tree_hook_kernel, tree_flatten_kernel, row_sums_kernel in the statistics).
Workloads: synth2500 = the 2,500 probands of tests/test_phi_tree_gpu.py; the others are those of profiles/gc_bench.py (cfg3: 1e4
probands; cfg4: 1e5 probands, a 40 GB matrix).
"""
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


def active_shares(n, row, col, kin):
    """The share of rows read in every round, replayed from the forest: in a round every component that still has a forest edge out
    picks its first one in list order (the list is in edge order), the picks are joined, and a component without one is finished."""
    comp = np.arange(n)
    done = np.zeros(n, dtype=bool)                               # by component root
    left = np.ones(len(row), dtype=bool)                         # forest edges not yet taken
    shares = []
    while True:
        shares.append(round(float(np.count_nonzero(~done[comp])) / n, 4))
        e = np.flatnonzero(left)
        a, b = comp[row[e]], comp[col[e]]
        first = np.full(n, len(row), dtype=np.int64)             # per component: its first edge out, in list order
        np.minimum.at(first, a, e)
        np.minimum.at(first, b, e)
        roots = np.flatnonzero((comp == np.arange(n)) & ~done)
        done[roots[first[roots] == len(row)]] = True
        take = np.unique(first[roots][first[roots] < len(row)])
        if not len(take):
            return shares
        left[take] = False
        for x, y in zip(comp[row[take]].tolist(), comp[col[take]].tolist()):      # join: the root of a component is its smallest position
            while comp[x] != x:
                x = int(comp[x])
            while comp[y] != y:
                y = int(comp[y])
            comp[max(x, y)] = min(x, y)
        while True:
            up = comp[comp]
            if np.array_equal(up, comp):
                break
            comp = up
        if not left.any() and len(row) == n - 1:                 # (the device stops there too; short of N - 1 it looks once more)
            return shares


def run(name, args):
    import genlib_jl_amd as gen
    ped, pro = load(name)
    L = gen._capi.lib()
    pl = gen.plan(ped, pro)
    try:
        pl.compute_device(device=0)
        n = pl.n_probands
        res = {"workload": name, "n_pro": n, "reps": args.reps, "copy_tbs": COPY_TBS}
        label = np.empty(n, np.int32)

        def clusters(t):
            k = C.c_int64()
            rc = L.genphi_result_clusters(pl._h, t, label.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(k), None)
            assert rc == 0, gen._capi.last_error()
            return k.value

        sums, per_floor = [], {}
        for name_f in args.floors:
            floor = None if name_f == "none" else float(name_f)
            t = gen._capi.tree_floor(floor)
            times = {"tree": [], "clusters": []}
            for rep in range(args.reps + 1):
                s_ms = _ms(pl.result_sums)[0]
                t_ms, (row, col, kin, n_trees, rounds) = _ms(lambda: pl.tree(floor))
                c_ms, k = _ms(lambda: clusters(t))
                assert k == n_trees
                if rep:                                          # (the first round is the warm-up)
                    sums.append(s_ms)
                    times["tree"].append(t_ms)
                    times["clusters"].append(c_ms)
            st = {key + "_ms": _stat(v) for key, v in times.items()}
            shares = active_shares(n, row, col, kin)
            st.update(floor=name_f, edges=len(row), trees=n_trees, rounds=rounds, per_round_ms=round(st["tree_ms"]["median"] / max(rounds, 1), 3),
                      active_share=shares, replayed_rounds=len(shares))
            per_floor[name_f] = st
        res["sums_ms"] = _stat(sums)
        res["sums_share"] = round(4.0 * n * n / (res["sums_ms"]["median"] * 1e-3) / (COPY_TBS * 1e12), 3)
        for st in per_floor.values():
            st["round_over_sums"] = round(st["per_round_ms"] / res["sums_ms"]["median"], 3)
        res["floors"] = per_floor
        print(json.dumps(res), flush=True)
    finally:
        pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["cfg3", "cfg4"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--floors", nargs="+", default=["none", str(1 / 1024), str(1 / 64), str(1 / 8)])
    args = ap.parse_args()
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
