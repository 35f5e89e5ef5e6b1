"""gen.simuUniqueness on one GPU: device time of the label sweep and of the count kernel, against gen.simuCarriers' sweep and count
kernel on the same probands in the same process (its count kernel decodes the same sides once per chunk of 608 labels, one dword per
cell; here a chunk is 1,216 labels of 16 bits and decodes the probands twice: the yardstick), the A/B of the two forms of the
attribute phase, and the A/B of the label chunks.

    python profiles/uniqueness_bench.py [--workload genea140 synth2000 synth10000 ...] [--simul 5000] [--reps 5] [--seed 7]

One JSON line per workload (what = "uniqueness"): plan_ms (host: UniquenessPlan), sweep_ms and count_ms of what ships (default chunk,
default form, max_share = 8 as gen.simuUniqueness passes it; each the median over --reps computes after one warm-up; HIP events,
genphi_unique_stats: init and level steps / count kernel, summed over the panels), count_bytes and count_gbs, n_live, levels,
n_labels, planes, columns, chunk_labels, chunks, lds_bytes, panel_cols, panels; from gen.CarriersPlan on the same probands as cases
(max_count = 8): carry_sweep_ms, carry_count_ms, carry_chunks, and count_over_carry = count_ms / carry_count_ms; invariant_sides: every
row of alleles + autozygous sums to 2 S; the forms: count_ms_form["plain"] (one atomic per lane) and ["ballot"] (the lanes of a wave
that meet in one of the first columns counted by a ballot), two handles of each, alternating, with forms_equal; the chunks:
count_ms_chunk["640"] (what an argument of 608 rounds up to) and ["1216"] with chunks_equal; the width: count_ms_full with every share
in its own column (max_share = 0), for at most 2,000 probands, with full_consistent: the table of 8 columns is the full one with its
tail summed.
Workloads: those of profiles/carriers_bench.py; the listed probands are the population, there are no others.
The forms are picked by the environment hook GENPHI_UNIQUE_ATTRIBUTE (1 = plain, 2 = ballot), which this script sets itself.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

os.environ["GENPHI_ENV_HOOKS"] = "1"         # (before the library reads it) the A/B of the attribute forms goes through a hook

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from ident_bench import load  # noqa: E402
from retain_bench import computes, med  # noqa: E402

FORMS = {"plain": "1", "ballot": "2"}


def run(name, args):
    import genlib_jl_amd as gen
    ped, pro = load(name)
    arrs = (ped.ind, ped.father, ped.mother, pro)
    gen._capi.lib().genphi_release_cached()

    def measure(form=None, **kw):
        os.environ.pop("GENPHI_UNIQUE_ATTRIBUTE", None)
        if form is not None:
            os.environ["GENPHI_UNIQUE_ATTRIBUTE"] = FORMS[form]
        kw.setdefault("max_share", 8)
        h = gen.UniquenessPlan(*arrs, simul_no=args.simul, seed=args.seed, **kw)
        os.environ.pop("GENPHI_UNIQUE_ATTRIBUTE", None)
        try:
            sweep, count, st = computes(h, args.reps, "count_ms")
            return sweep, count, st, (h.alleles_to_host(), h.autozygous_to_host()), h
        finally:
            h.close()

    t0 = time.perf_counter()
    gen.UniquenessPlan(*arrs, simul_no=args.simul, seed=args.seed, max_share=8).close()
    plan_ms = (time.perf_counter() - t0) * 1e3
    sweep, count, st, out, h = measure()
    n = st["n"]
    res = {"workload": name, "what": "uniqueness", "n_ind": len(ped), "n": n, "n_pop": st["n_pop"], "simul": args.simul, "n_live": h.n_live,
           "levels": st["levels"], "n_labels": h.n_labels, "planes": st["planes"], "columns": st["columns"], "chunk_labels": st["chunk_labels"],
           "chunks": st["chunks"], "lds_bytes": st["lds_bytes"], "panel_cols": st["panel_cols"], "panels": st["panels"], "plan_ms": round(plan_ms, 3),
           "sweep_ms": med(sweep), "sweep_ms_all": [round(t, 4) for t in sweep], "count_ms": med(count), "count_ms_all": [round(t, 4) for t in count],
           "algorithmic_bytes": st["algorithmic_bytes"], "count_bytes": st["count_bytes"]}
    res["count_gbs"] = round(st["count_bytes"] / res["count_ms"] / 1e6, 1) if res["count_ms"] else None
    res["invariant_sides"] = bool(np.all(out[0].sum(axis=1, dtype=np.int64) + out[1].sum(axis=1, dtype=np.int64) == 2 * args.simul))
    c = gen.CarriersPlan(*arrs, simul_no=args.simul, seed=args.seed, max_count=8)
    try:
        s, k, cs = computes(c, args.reps, "count_ms")
        res["carry_sweep_ms"], res["carry_count_ms"], res["carry_chunks"] = med(s), med(k), cs["chunks"]
    finally:
        c.close()
    res["count_over_carry"] = round(res["count_ms"] / res["carry_count_ms"], 3) if res["carry_count_ms"] else None
    times, equal = {form: [] for form in FORMS}, True
    for _ in range(2):                                                   # alternating: a drift of the clock falls on both
        for form in FORMS:
            _, k, _, o, _ = measure(form=form)
            times[form] += k
            equal = equal and all(np.array_equal(a, b) for a, b in zip(out, o))
    res["count_ms_form"] = {form: med(t) for form, t in times.items()}
    res["forms_equal"] = equal
    res["count_ms_chunk"], res["chunks_forced"], equal = {}, {}, True
    for lc in (608, 1216):
        _, k, s2, o, _ = measure(chunk_labels=lc)
        res["count_ms_chunk"][str(s2["chunk_labels"])] = med(k)
        res["chunks_forced"][str(s2["chunk_labels"])] = s2["chunks"]
        equal = equal and all(np.array_equal(a, b) for a, b in zip(out, o))
    res["chunks_equal"] = equal
    if n <= 2000:
        _, k, s2, o, _ = measure(max_share=0)
        res["count_ms_full"], res["columns_full"] = med(k), s2["columns"]
        res["full_consistent"] = bool(all(np.array_equal(a[:, :7], b[:, :7]) and np.array_equal(a[:, 7], b[:, 7:].sum(axis=1)) for a, b in zip(out, o)))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["genea140", "synth2000", "synth10000"])
    ap.add_argument("--simul", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    for name in args.workload:
        run(name, args)


if __name__ == "__main__":
    main()
