"""gen.simuOrigins on one GPU: device time of the label sweep and of the count kernel at one group and at seven, against
gen.simuCarriers' sweep and count kernel on the same probands in the same process (it decodes the same sides: the yardstick, per
chunk and as whole kernels), against gen.simuIdentity's pair kernel (the O(N^2) route to the same group sums), and the A/B of the
label chunks: the default (the widest) against half of it, two workgroups per CU.

    python profiles/origins_bench.py [--workload genea140 synth2000 synth10000 ...] [--simul 5000] [--reps 5] [--seed 7] [--ident-max 10000]

One JSON line per workload (what = "origins"): plan_ms (host: OriginsPlan); per G in g1 / g7 (genea140: the 7 populations of
tests/golden/pop140.csv; synthetic: proband i in group i mod 7): sweep_ms and count_ms (each the median over --reps computes after one
warm-up; HIP events, genphi_origin_stats: init and level steps / count kernel, summed over the panels), chunk_labels, chunks,
lds_bytes, count_ms_per_chunk, count_ms_half (chunk_labels // 2) with chunks_half and half_equal, by_proband_count_ms; from
gen.CarriersPlan on the same probands: carry_sweep_ms, carry_count_ms, carry_chunks, carry_count_ms_per_chunk; the ratios
count_over_carry (whole kernels) and count_over_carry_per_chunk; sweep_over_carry_sweep; from gen.IdentityPlan (skipped above
--ident-max probands): ident_pair_ms and pair_over_count; merged_agree: the seven groups merged give the one-group tables; invariant_copies:
the copies of every group sum to 2 n_a S.
Workloads: those of profiles/ident_bench.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from ident_bench import computes as ident_computes, load  # noqa: E402
from retain_bench import computes, med  # noqa: E402


def groups_of(name, pro):
    import genlib_jl_amd as gen
    if name == "genea140":
        pop = gen._pop(os.path.join(ROOT, "tests", "golden", "pop140.csv"))
        names = sorted(set(pop.values()))
        return np.array([names.index(pop[int(p)]) for p in pro.tolist()], dtype=np.int32)
    return (np.arange(len(pro)) % 7).astype(np.int32)


def run(name, args):
    import genlib_jl_amd as gen
    ped, pro = load(name)
    arrs = (ped.ind, ped.father, ped.mother, pro)
    seven = groups_of(name, pro)
    gen._capi.lib().genphi_release_cached()

    def measure(groups, G, **kw):
        h = gen.OriginsPlan(*arrs, groups, n_groups=G, simul_no=args.simul, seed=args.seed, **kw)
        try:
            sweep, count, st = computes(h, args.reps, "count_ms")
            return sweep, count, st, (h.copies_to_host(), h.autozygous_to_host(), h.matches_to_host()), h
        finally:
            h.close()

    t0 = time.perf_counter()
    gen.OriginsPlan(*arrs, seven, n_groups=7, simul_no=args.simul, seed=args.seed).close()
    plan_ms = (time.perf_counter() - t0) * 1e3
    res = {"workload": name, "what": "origins", "n_ind": len(ped), "n_pro": len(pro), "simul": args.simul, "plan_ms": round(plan_ms, 3)}
    c = gen.CarriersPlan(*arrs, simul_no=args.simul, seed=args.seed)
    try:
        s, k, cs = computes(c, args.reps, "count_ms")
        res.update(carry_sweep_ms=med(s), carry_sweep_ms_all=[round(t, 4) for t in s], carry_count_ms=med(k), carry_chunks=cs["chunks"],
                   carry_count_ms_per_chunk=round(med(k) / cs["chunks"], 5))
    finally:
        c.close()
    outs = {}
    for key, groups, G in (("g1", None, 1), ("g7", seven, 7)):
        sweep, count, st, out, h = measure(groups, G)
        outs[key] = out
        r = {"sweep_ms": med(sweep), "sweep_ms_all": [round(t, 4) for t in sweep], "count_ms": med(count), "count_ms_all": [round(t, 4) for t in count],
             "chunk_labels": st["chunk_labels"], "chunks": st["chunks"], "lds_bytes": st["lds_bytes"], "count_bytes": st["count_bytes"],
             "count_ms_per_chunk": round(med(count) / st["chunks"], 5)}
        r["count_over_carry"] = round(r["count_ms"] / res["carry_count_ms"], 3)
        r["count_over_carry_per_chunk"] = round(r["count_ms_per_chunk"] / res["carry_count_ms_per_chunk"], 3)
        r["sweep_over_carry_sweep"] = round(r["sweep_ms"] / res["carry_sweep_ms"], 3)
        _, half, hs, o, _ = measure(groups, G, chunk_labels=max(1, st["chunk_labels"] // 2))
        r.update(count_ms_half=med(half), chunks_half=hs["chunks"], lds_bytes_half=hs["lds_bytes"], half_equal=bool(all(np.array_equal(a, b) for a, b in zip(out, o))))
        _, byp, _, o, _ = measure(groups, G, by_proband=True)
        r.update(by_proband_count_ms=med(byp), by_proband_equal=bool(all(np.array_equal(a, b) for a, b in zip(out, o))))
        sizes = np.bincount(np.zeros(len(pro), dtype=np.int64) if groups is None else groups, minlength=G)
        r["invariant_copies"] = bool(np.array_equal(out[0].sum(axis=1), 2 * sizes * args.simul))
        res[key] = r
        res.update(n_live=h.n_live, levels=st["levels"], n_labels=h.n_labels, planes=st["planes"], panel_cols=st["panel_cols"], panels=st["panels"])
    res["merged_agree"] = bool(np.array_equal(outs["g7"][0].sum(axis=0), outs["g1"][0][0]) and np.array_equal(outs["g7"][1].sum(axis=0), outs["g1"][1][0]) and
                               np.array_equal(outs["g7"][2].sum(axis=0), outs["g1"][2][0]))
    if len(pro) <= args.ident_max:
        g = gen.IdentityPlan(*arrs, simul_no=args.simul, seed=args.seed)
        try:
            _, pair, _ = ident_computes(g, max(1, args.reps // 2))
            res["ident_pair_ms"] = med(pair)
            res["pair_over_count_g7"] = round(res["ident_pair_ms"] / res["g7"]["count_ms"], 2)
            cnt = g.counts_to_host().astype(np.int64)
            num = np.triu(4 * cnt[..., 0] + 2 * (cnt[..., 2] + cnt[..., 4] + cnt[..., 6]) + cnt[..., 7], 1).sum()
            res["ident_agrees"] = bool(num == outs["g1"][2].sum())
        finally:
            g.close()
    else:
        res["ident_pair_ms"] = None
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["genea140", "synth2000", "synth10000"])
    ap.add_argument("--simul", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--ident-max", type=int, default=10000)
    args = ap.parse_args()
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
