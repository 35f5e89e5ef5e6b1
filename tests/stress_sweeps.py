"""Random differential stress of the five ancestor sweeps on the GPU (not part of the pytest run by itself; tests/test_sweeps_random.py
runs a short fixed-seed round of it):
    python tests/stress_sweeps.py [n_cases] [seed]
Random pedigrees x proband lists x ancestor lists x panel widths (every lanes-per-row form of every kernel) x panels per launch x
occ's row width, and for each case gen.gc, gen.occ (IND and TOTAL), gen.rec, gen.meioses, gen.findMRCA, gen.findFounders,
gen.completeness (IND, MEAN, counts, totals of both kinds of handle) and gen.depth against the Python oracles of tests/*_oracle.py.
No tolerance anywhere: the cases stay inside the ranges where the library claims identity (sweeps of at most 52 steps,
25 * totals < 2^53), and every handle is computed twice.  Prints one `FAIL case=...` line per failing case with everything needed to
replay it (tests/sweep_case.py <case>), and a summary."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
os.environ["GENPHI_ENV_HOOKS"] = "1"      # the knobs below are environment hooks: read by the library only under this gate

KNOBS = ["GENPHI_GC_PANEL", "GENPHI_GC_PANELS_PER_LAUNCH", "GENPHI_OCC_PANEL", "GENPHI_OCC_PANELS_PER_LAUNCH", "GENPHI_OCC_ROWS",
         "GENPHI_DIST_PANEL", "GENPHI_DIST_PANELS_PER_LAUNCH"]

MAX_STEPS = 52                # gc: Float64 rows are exact up to here
RANDOM_MAX_DEPTH = 36         # generations of a random_pedigree draw: 25 * 600 probands * 2^35 < 2^53
LITERAL_MAX_STEPS = 24        # gc_literal (Float32 path sums) is exact up to here ...
LITERAL_MAX_PATHS = 300_000   # ... and walks one path at a time

# Panel widths that between them select every lanes-per-row instantiation (1, 2, 4, ..., 64) of a family's kernels, with odd widths, widths
# that are no multiple of 8 and (dist) panels that start off a multiple of 8 columns.  The rule (lanes_per_row in csrc/sweep_device.h) and its arguments:
#   gc        the power of two >= ceil(C / 2) pairs of Float64 columns
#   occ       >= ceil(C / 4) vectors of 32-bit counts, ceil(C / 2) of 64-bit counts;  rec: >= ceil(C / 128) vectors of two 64-column words
#   meioses   >= ceil(C / 8) vectors of eight 16-bit entries
GC_PANELS = [1, 2, 3, 4, 5, 7, 8, 9, 13, 16, 17, 30, 32, 33, 50, 64, 65, 100, 128, 131]
OCC_PANELS = [1, 3, 4, 5, 8, 11, 16, 17, 32, 33, 64, 65, 100, 128, 129, 200, 256, 300]
DIST_PANELS = [1, 3, 8, 9, 16, 20, 32, 40, 64, 65, 72, 128, 130, 256, 257, 300]
REC_WIDE_PANELS = [128, 640, 1100, 2100, 4096]          # every individual as an ancestor: several panels of bit rows
PER_LAUNCH = [None, 1, 2, 7]


def lanes_per_row(vectors):
    lpr = 1
    while lpr < vectors and lpr < 64:
        lpr *= 2
    return lpr


def gc_lanes(cols):
    return lanes_per_row((cols + 1) // 2)


def occ_lanes(cols, row_bits):
    per = 16 // (row_bits // 8)
    return lanes_per_row((cols + per - 1) // per)


def rec_lanes(cols):
    words = (cols + 63) // 64
    return lanes_per_row((words + 1) // 2)


def dist_lanes(cols):
    return lanes_per_row((cols + 7) // 8)


def make_case(case):
    """Everything of one random case, a pure function of `case`: dict(kind, ind, father, mother, sex, sort, pro, anc, rec_pro, ids, env)."""
    from genlib_jl_amd import synth
    from random_pedigree import random_pedigree
    r = np.random.default_rng([case, 17])
    u = r.random()
    if u < 0.45:
        kind = "mating"
        n_gen = int(r.integers(3, 16))
        n_pro = int(r.integers(5, 200))
        n_ind = n_pro + (n_gen - 1) * int(r.integers(20, 340))
        skip = int(r.choice([0, 0, 30, 150, 400, 650, 850]))
        ind, fa, mo, sex, _ = synth.random_mating(n_ind, n_pro, n_gen, seed=case, skip_permille=skip)
        if r.random() < 0.4:                                              # one-parent members
            fa, mo = fa.copy(), mo.copy()
            k = np.arange(len(ind))
            mo[(k % int(r.integers(7, 40)) == 5) & (fa != 0)] = 0
            fa[(k % int(r.integers(7, 40)) == 3) & (mo != 0)] = 0
    elif u < 0.85:
        kind = "random"
        n = int(r.choice([30, 120, 400, 900, 1500]))
        pf, p1, ps = float(r.choice([0.01, 0.05, 0.3])), float(r.choice([0.0, 0.1, 0.3])), float(r.choice([0.0, 0.05]))
        back = int(r.choice([5, 50, 400, n]))
        ind, fa, mo, sex = random_pedigree(r, n, pf, p1, ps, back, max_depth=RANDOM_MAX_DEPTH)
    else:
        kind = "deep"                                                     # 33 - 52 generations: occ goes from 32- to 64-bit rows at 31 steps
        n_gen = int(r.integers(33, 53))
        per = int(r.integers(12, 60))
        ind, fa, mo, sex, _ = synth.deep_inbred(n_gen, per, int(r.integers(2, 5)), seed=case)
        mo = mo.copy()
        mo[(np.arange(len(ind)) // per) % 4 == 2] = 0                     # every fourth generation has no mothers: at most 2^39 paths, inside Float64
    n = len(ind)
    sort = bool(r.random() < 0.6)
    if not sort:
        ind, fa, mo, sex = synth.parents_first_shuffle(ind, fa, mo, sex, seed=case & 0xffff)
    parents = np.union1d(fa, mo)
    leaves = np.setdiff1d(ind, parents)
    founders = ind[(fa == 0) & (mo == 0)]
    nonleaf = np.setdiff1d(ind, leaves)
    nonfounder = np.setdiff1d(ind, founders)

    def some(pool, k):
        return r.choice(pool, size=min(int(k), len(pool)), replace=False) if len(pool) and k > 0 else np.zeros(0, dtype=np.int64)

    # probands, in the style of _mixed_lists (tests/test_gc_gpu.py)
    u = r.random()
    if u < 0.10 and n <= 600:
        pro = ind.copy() if r.random() < 0.5 else r.permutation(ind)      # every individual
    elif u < 0.17:
        pro = some(founders, r.integers(1, 12))                           # founders only: one cut
        pro = np.concatenate([pro, pro[:1]])
    elif u < 0.30:
        pro = some(leaves, r.integers(1, 200))
    else:
        pro = np.concatenate([some(leaves, r.integers(1, 150)), some(nonleaf, r.integers(0, 12)), some(founders, r.integers(0, 5))])
        pro = np.concatenate([pro, r.choice(pro, size=int(r.integers(0, 5)))])
        pro = r.permutation(pro)
    pro = np.asarray(pro, dtype=np.int64)
    # ancestors: founders, non-founders, a proband, a founder without children, repeats; a length that leaves the panels ragged
    wide = r.random() < 0.08 and len(pro) <= 60
    if wide:
        anc = r.permutation(ind)                                          # every individual as an ancestor
    else:
        u = r.random()
        n_anc = int(r.integers(1, 21)) if u < 0.2 else int(r.integers(21, 131)) if u < 0.6 else int(r.integers(131, 351))
        pool = np.concatenate([some(founders, r.integers(1, n_anc + 1)), some(nonfounder, r.integers(0, n_anc // 3 + 2)), pro[:1],
                               some(np.intersect1d(founders, leaves), 1)])
        pool = r.permutation(pool)[:n_anc]
        if len(pool) < n_anc:
            pool = np.concatenate([pool, r.choice(pool, size=n_anc - len(pool))])            # repeats
        elif n_anc >= 3 and r.random() < 0.5:
            pool[-1] = pool[0]
        anc = r.permutation(pool)
    anc = np.asarray(anc, dtype=np.int64)
    rec_pro = np.concatenate([pro, [int(ind.max()) + 12345]]) if r.random() < 0.3 else pro           # rec ignores unknown probands
    distinct = np.unique(pro)
    ids = r.permutation(distinct)[: int(r.integers(2, 7))]                # findMRCA / findFounders: a few of the probands
    env = {}
    if r.random() < 0.8:
        env["GENPHI_GC_PANEL"] = str(int(r.choice(GC_PANELS)))
    if r.random() < 0.8:
        env["GENPHI_OCC_PANEL"] = str(int(r.choice(REC_WIDE_PANELS if wide else OCC_PANELS)))
    if r.random() < 0.8:
        env["GENPHI_DIST_PANEL"] = str(int(r.choice(DIST_PANELS)))
    for fam in ("GC", "OCC", "DIST"):
        g = PER_LAUNCH[int(r.integers(0, 4))]
        if g is not None:
            env["GENPHI_%s_PANELS_PER_LAUNCH" % fam] = str(g)
    if r.random() < 0.25:
        env["GENPHI_OCC_ROWS"] = "64"
    return dict(kind=kind, ind=ind, father=fa, mother=mo, sex=sex, sort=sort, pro=pro, anc=anc, rec_pro=rec_pro, ids=ids, env=env)


def describe(c):
    return "kind=%s n_ind=%d n_pro=%d n_anc=%d sort=%s env=%s" % (c["kind"], len(c["ind"]), len(c["pro"]), len(c["anc"]), c["sort"], c["env"])


def oracles(c, ind, fa, mo):
    """The expected results of a case from the Python oracles, on the pedigree arrays in rank order."""
    from completeness_oracle import completeness_exact, depth_exact, mean_fraction
    from gc_oracle import gc_exact_rows, gc_literal
    from mrca_oracle import find_founders_exact, find_mrca_exact, meioses_exact
    from occ_oracle import occ_exact, rec_exact
    pro, anc = c["pro"], c["anc"]
    depth = depth_exact(ind, fa, mo)
    assert depth - 1 <= MAX_STEPS, "the generator left the exact range of gen.gc: %d steps" % (depth - 1)
    want = {"depth": depth, "gc": gc_exact_rows(ind, fa, mo, pro, anc)}
    # the literal path sums where they are exact and affordable: paths below an ancestor = paths below its children, 1 for a leaf
    pos = {int(x): k for k, x in enumerate(ind)}
    below = [0] * len(ind)
    has_child = [False] * len(ind)
    for k in range(len(ind) - 1, -1, -1):                                 # rank order: children after parents
        if not has_child[k]:
            below[k] = 1
        for q in (fa[k], mo[k]):
            if q:
                below[pos[int(q)]] += below[k]
                has_child[pos[int(q)]] = True
    paths = sum(below[pos[int(a)]] for a in anc)
    if depth - 1 <= LITERAL_MAX_STEPS and paths <= LITERAL_MAX_PATHS:
        want["gc_literal"] = gc_literal(ind, fa, mo, pro, anc)
    want["occ"] = occ_exact(ind, fa, mo, pro, anc)
    want["occ_total"] = want["occ"].sum(axis=1, dtype=np.int64)           # modulo 2^64, as the oracle's "TOTAL"
    want["rec"] = rec_exact(ind, fa, mo, c["rec_pro"], anc)
    want["meioses"] = meioses_exact(ind, fa, mo, pro, anc)
    want["mrca"] = find_mrca_exact(ind, fa, mo, c["ids"])
    want["founders"] = find_founders_exact(ind, fa, mo, c["ids"])
    counts, matrix = completeness_exact(ind, fa, mo, pro)
    assert counts.dtype == np.int64
    totals = [sum(int(v) for v in counts[:, g]) for g in range(counts.shape[1])]
    assert all(25 * t < 2 ** 53 for t in totals), "the generator left the exact range of gen.completeness MEAN"
    want["comp_counts"], want["comp_ind"] = counts, matrix
    want["comp_totals"] = np.asarray(totals, dtype=np.int64)
    want["comp_mean"] = np.array([[float(f)] for f in mean_fraction(counts)])
    return want


def _differs(got, want, bits=False):
    """None when equal (shape, dtype, every entry; bits: Float32 bit patterns), else a short description of the difference."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "shape / dtype %s %s, expected %s %s" % (got.shape, got.dtype, want.shape, want.dtype)
    a, b = (got.view(np.int32), want.view(np.int32)) if bits else (got, want)
    bad = np.argwhere(a != b)
    if len(bad) == 0:
        return None
    first = tuple(int(v) for v in bad[0])
    rows = np.unique(bad[:, 0])[:8].tolist()
    cols = np.unique(bad[:, -1])[:8].tolist()
    return "%d of %d entries differ; first at %s: %r, expected %r; rows %s, columns %s" % (len(bad), got.size, first, got[first], want[first], rows, cols)


def run_case(case, gen, report=None):
    """One case end to end.  Returns (list of the comparisons that failed, the case).  report: a function that gets one line per
    comparison (tests/sweep_case.py)."""
    c = make_case(case)
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(c["env"])
    what = []

    def check(name, got, want, bits=False):
        d = _differs(got, want, bits)
        if report:
            report("  %-28s %s" % (name, "ok" if d is None else d))
        if d is not None:
            what.append(name)

    try:
        ped = gen.genealogy({"ind": c["ind"], "father": c["father"], "mother": c["mother"], "sex": c["sex"]}, sort=c["sort"])
        args = (ped.ind, ped.father, ped.mother)
        want = oracles(c, *args)
        pro, anc = c["pro"], c["anc"]
        check("depth", np.array([gen.depth(ped)], dtype=np.int64), np.array([want["depth"]], dtype=np.int64))
        for again in ("", " (second compute)"):                           # every handle twice: buffer reuse and the result pre-fill
            if again == "":
                gc = gen.GCPlan(*args, pro, anc)
                occ = gen.OccPlan(*args, pro, anc)
                tot = gen.OccPlan(*args, pro, anc, total_only=True)
                rec = gen.RecPlan(*args, c["rec_pro"], anc)
                dist = gen.DistPlan(*args, pro, anc)
                comp = gen.CompletenessPlan(*args, pro)
                ctot = gen.CompletenessPlan(*args, pro, totals_only=True)
                handles = [gc, occ, tot, rec, dist, comp, ctot]
            for h in handles:
                h.compute()
            out = gc.result_to_host()
            check("gc" + again, out, want["gc"], bits=True)
            if "gc_literal" in want:
                check("gc vs literal" + again, out, want["gc_literal"], bits=True)
            check("occ IND" + again, occ.result_to_host().T, want["occ"])
            check("occ totals of IND" + again, occ.totals(), want["occ_total"])
            check("occ TOTAL" + again, tot.totals(), want["occ_total"])
            check("rec" + again, rec.result(), want["rec"])
            check("meioses" + again, dist.result_to_host(), want["meioses"])
            check("completeness counts" + again, comp.counts(), want["comp_counts"])
            check("completeness IND" + again, comp.result_to_host().T, want["comp_ind"])
            check("completeness totals of IND" + again, comp.totals(), want["comp_totals"])
            check("completeness totals only" + again, ctot.totals(), want["comp_totals"])
            if report and again == "":
                report("  panels: gc %s, occ %s (%d-bit rows), rec %s, meioses %s; steps <= %d" % (
                    gc.stats()["panel_cols"], occ.stats()["panel_cols"], occ.stats()["row_bits"], rec.stats()["panel_cols"],
                    dist.stats()["panel_cols"], want["depth"] - 1))
        for h in handles:
            h.close()
        check("completeness MEAN", gen.completeness(ped, pro), want["comp_mean"])
        check("completeness IND (gen.completeness)", gen.completeness(ped, pro, type="IND"), want["comp_ind"])
        m = gen.findMRCA(ped, c["ids"])
        check("findMRCA ancestors", m.ancestors, want["mrca"][0])
        check("findMRCA meioses", m.meioses, want["mrca"][1])
        check("findFounders", gen.findFounders(ped, c["ids"]), want["founders"])
    except Exception as e:          # noqa: BLE001
        what.append("exception %s: %s" % (type(e).__name__, e))
        if report:
            report("  " + what[-1])
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
    return what, c


def main():
    import genlib_jl_amd as gen
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 120
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 12345
    rng = np.random.default_rng(seed0)
    t0, n_fail = time.time(), 0
    for k in range(n_cases):
        case = int(rng.integers(1 << 30))
        what, c = run_case(case, gen)
        if what:
            n_fail += 1
            print("FAIL case=%d %s -> %s" % (case, describe(c), what), flush=True)
        if (k + 1) % 20 == 0:
            print("... %d cases, %d failures, %.0f s" % (k + 1, n_fail, time.time() - t0), flush=True)
    print("sweep stress: %d cases, %d failures in %.0f s (seed %d)" % (n_cases, n_fail, time.time() - t0, seed0), flush=True)
    return 1 if n_fail else 0


if __name__ == "__main__":
    sys.exit(main())
