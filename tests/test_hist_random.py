"""genphi_result_hist / genphi_result_select over every path that delivers the resident result: 40 fixed-seed cases drawn with the
generators of tests/stress_queries.py (the pedigrees, proband lists and sweep knobs of tests/stress_random.py: FULL / SPLIT / WIDE last
steps, a result delivered from the slot matrix, sparse leading cuts, unaligned, one-row and empty shards, a Float64 result in between,
a device cache soiled with positive floats).  After every resident state: the histogram without and with labels over random edges,
and the entries of 1 - 16 random ranks, against tests/phi_hist_oracle.py on the host copy of the same state, ==.  One test without a
GPU checks that the round reaches every delivery path."""
import numpy as np
import pytest

import phi_hist_oracle as HO
import stress_queries as S

ROUND_CASES, ROUND_SEED, PARTS = 40, 20261019, 4


def _round():
    rng = np.random.default_rng(ROUND_SEED)
    return [int(rng.integers(1 << 30)) for _ in range(ROUND_CASES)]


def _edges(r, host):
    """Random strictly increasing edges: uniform, on values of the data, or powers of two; sometimes infinite outer edges."""
    kind = int(r.integers(3))
    if kind == 0:
        e = np.linspace(0.0, float(r.choice([0.5, 0.0625, 1.0])), int(r.choice([1, 7, 64, 1000])) + 1)
    elif kind == 1 and host.size:
        v = np.unique(host.astype(np.float64))
        pick = np.unique(r.choice(v, size=min(len(v), int(r.integers(1, 9))), replace=False))
        e = np.unique(np.concatenate([pick, np.nextafter(pick[:1], np.inf), [float(v.max()) + 1.0]]))
    else:
        e = 2.0 ** np.arange(-int(r.integers(2, 31)), 1.0)
    if r.random() < 0.25:
        e = np.concatenate([[-np.inf], e])
    if r.random() < 0.25:
        e = np.concatenate([e, [np.inf]])
    return e


def _one_case(gen, case):
    c = S.make_case(case)
    n = c["n"]
    what = []
    ind, fa, mo, sex = c["ind"], c["father"], c["mother"], c["sex"]
    if not c["sort"]:
        from genlib_jl_amd import synth
        ind, fa, mo, sex = synth.parents_first_shuffle(ind, fa, mo, sex, seed=c["base"] & 0xffff)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}, sort=c["sort"])
    if c["soil"]:
        assert S.soil(gen, n)
    pl = gen.plan(ped, c["pro"], tuning=c["tuning"])
    try:
        for s in c["states"]:
            r0, r1 = S.rows_of(s, n)
            if s["release"]:
                pl.release_device()
            pl.compute_device(kernel=s["kernel"], rows=s["rows"], storage64=s["f64"], no_sparse=s["no_sparse"])
            r = np.random.default_rng([case, s["label_seed"]])
            if s["f64"]:
                for call in (lambda: pl.hist([0.0, 0.5]), lambda: pl.select([0]), lambda: pl.count_pairs()):
                    with pytest.raises(ValueError):
                        call()
                continue
            host = pl.result_to_host()
            assert host.shape == (r1 - r0, n)
            pairs = HO.n_pairs(n, r0, r1)
            if pl.count_pairs() != pairs:
                what.append("%s: count_pairs" % S.show_state(s))
            edges = _edges(r, host)
            if not HO.same(pl.hist(edges), HO.hist(host, edges, row_begin=r0)):
                what.append("%s: hist, %d edges" % (S.show_state(s), len(edges)))
            g = min(s["G"], 256)
            for name, lab in zip(("runs", "any"), S.labels_of(s, n)):
                lab = np.where(lab >= g, -1, lab).astype(np.int32)
                e = edges if g * (len(edges) - 1) <= 16384 else edges[:16384 // g + 1]
                if not HO.same(pl.hist(e, lab, g), HO.hist(host, e, lab, g, row_begin=r0)):
                    what.append("%s: hist %s G=%d, %d edges" % (S.show_state(s), name, g, len(e)))
            if pairs:
                ranks = r.integers(0, pairs, int(r.integers(1, 17)))
                ranks[0] = int(r.choice([0, pairs - 1, pairs // 2]))
                got, ref = pl.select(ranks), HO.select(host, ranks, row_begin=r0)
                if not np.array_equal(got.view(np.uint32), ref.view(np.uint32)):
                    what.append("%s: select %s" % (S.show_state(s), ranks.tolist()))
            else:
                with pytest.raises(ValueError):
                    pl.select([0])
    finally:
        pl.close()
    return ["case %d (%s): %s" % (case, S.describe(c), w) for w in what]


def test_the_round_reaches_every_delivery_path(gen):
    """A check of the round itself, not of the kernels (no GPU): the plan of every case, built on the host, and its state list
    fall into the classes tests/test_queries_random.py names for its own round (its classes_of is imported: one definition of the
    delivery paths).  Every class is met, and the plan has the methods the round calls."""
    from test_queries_random import CLASSES, classes_of
    assert all(callable(getattr(gen.PhiPlan, name)) for name in ("hist", "select", "count_pairs"))
    seen = {k: 0 for k in CLASSES}
    for case in _round():
        for k in classes_of(gen, S.make_case(case)):
            seen[k] += 1
    print(seen)
    assert all(v >= 1 for v in seen.values()), seen


@pytest.mark.gpu
@pytest.mark.parametrize("part", range(PARTS))
def test_hist_and_select_over_random_resident_states(gen, part):
    """10 of the 40 cases; no case is skipped."""
    cases = _round()[part::PARTS]
    assert len(cases) == ROUND_CASES // PARTS
    failures = []
    for case in cases:
        failures += _one_case(gen, case)
    assert not failures, "\n".join(failures)
