"""The three gene-dropping sweeps (gen.simuSample / gen.simuProb, gen.simuIdentity, gen.simuSharing) where the pinned shapes of
tests/test_simu_gpu.py, tests/test_ident_gpu.py and tests/test_link_gpu.py do not reach: a short fixed-seed round of
tests/stress_drops.py, a host-only pass over the same round that counts what it reaches and compares every host plan with the
references', and the smallest shapes that show the two halves of the IDs and of the seed.  The step kernels key their Philox streams
on the low and the high 32 bits of the individual's ID and of the seed, four arguments of their own; in every other GPU test the two
high halves are zero.  Every comparison is np.array_equal with the references of tests/simu_oracle.py, tests/ident_oracle.py and
tests/link_oracle.py."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

import stress_drops as D
from ident_oracle import IdentVector, counts_of
from link_oracle import LinkVector, sums_of
from simu_oracle import SimuVector, match_counts, state_counts

HERE = os.path.dirname(os.path.abspath(__file__))
ROUND = (60, 20261042)            # the cases and the seed of the short round
FAILED_ONCE = ()                   # (case, ...): every case number a round of tests/stress_drops.py ever failed


def _same(got, want):
    d = D._differs(got, want)
    assert d is None, d


@pytest.mark.gpu
def test_drop_stress_short():
    """60 fixed-seed cases of tests/stress_drops.py: random pedigrees (random mating with skipped generations and one-parent members,
    arbitrary pedigrees with founders anywhere, half-founders and selfing, inbred pedigrees of 33 - 52 generations) in file or rank
    order x four ID maps x four kinds of seed x mixed proband lists x, per family, simulations at the word and pair edges, forced
    and ragged panels, chromosomes at the word edges and the flags; the handles (computed twice) or the public functions, now and then
    with a fresh seed; every result against its reference.  No case is skipped.  Measured on an MI355X machine (one run): the
    references take 3.1 s of CPU for the 60 cases and the whole round 4.0 s of wall time (40 cases: 2.2 s and 2.8 s)."""
    n, seed = ROUND
    out = subprocess.run([sys.executable, os.path.join(HERE, "stress_drops.py"), str(n), str(seed)], cwd=HERE, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    last = out.stdout.splitlines()[-1]
    assert last.startswith("drop stress: %d cases, 0 failures" % n), out.stdout[-3000:]
    assert ", 0 failures" in last


# at least 3 cases of the short round in every one of these (stress_drops.classes)
CLASSES = (["simu lanes %d" % f for f in D.FORMS] + ["ident lanes %d" % f for f in D.FORMS] + ["link lanes %d" % f for f in D.LINK_FORMS] + [
    "simu one panel", "simu several panels", "simu ragged last panel", "simu S % 64 != 0", "simu S % 16 == 0, S % 64 != 0", "simu no_sample",
    "simu proband outside the live set", "simu proband that is a listed ancestor", "simu no live row",
    "ident one panel", "ident several panels", "ident ragged last panel", "ident n_pro <= 32", "ident n_pro 33 .. 64", "ident n_pro > 64",
    "ident n_pro % 32 == 0", "ident all_pairs", "ident labels off", "ident n_labels at a power of two", "ident n_labels below a power of two",
    "ident n_labels above a power of two",
    "link odd W", "link L % 64 == 0", "link L % 64 == 1", "link q = 0", "link q = 32768", "link q with several bits",
    "link several panels, ragged last",
    "sort=True", "sort=True, the rank order is not the file order", "sort=False", "api handles", "api wrappers", "fresh seed"] + ["ids " + m for m in D.ID_MAPS] + ["seed " + k for k in D.SEED_KINDS] + [
    fam + what for fam in ("simu", "ident", "link") for what in (" repeated probands", " everyone a proband", " selfing", " half-founder", " 30 levels")])


def test_the_short_round_reaches_every_class(gen):
    """No GPU.  Every case of the short round: make_case is a pure function of the case number; the three handles are planned (nothing
    is computed) and their host plans (live set, levels, rows per level, the planned rows of gen.SimuPlan, the allele tables and the
    planes) equal the references'; an ID map that shares low halves has full sibs that share one; and at least 3 cases fall in every
    class of CLASSES, derived from the case, the handles' host accessors and the references' plans."""
    seen = collections.Counter()
    for case in D.round_cases(*ROUND):
        c = D.make_case(case)
        assert D.describe(c) == D.describe(D.make_case(case))
        ped = D.genealogy(c, gen)
        args = (ped.ind, ped.father, ped.mother)
        if c["sort"]:
            assert np.array_equal(np.sort(ped.ind), np.sort(c["ind"]))
            seen.update(["sort=True, the rank order is not the file order"] * (not np.array_equal(ped.ind, c["ind"])))
        else:
            assert np.array_equal(ped.ind, c["ind"])
        if c["id_map"] == "low_shared":
            assert D.full_sibs_sharing_a_low_half(c["ind"], c["father"], c["mother"]) >= 2
        if c["id_map"] != "small":
            assert int(c["ind"].max()) >> 32 > 0
        refs = D.references(c, args)
        hs = D.handles(c, gen, args)
        try:
            for fam, name, got, want in D.plan_checks(c, args, *hs, *refs):
                d = D._differs(got, want)
                assert d is None, (case, fam, name, d)
            seen.update(D.classes(c, *hs, *refs))
        finally:
            for h in hs:
                h.close()
    print("\n".join("%3d %s" % (seen[k], k) for k in CLASSES))
    assert all(k in CLASSES or k.startswith(("pro ", "link n_pro")) for k in seen), sorted(set(seen) - set(CLASSES))
    short = {k: seen[k] for k in CLASSES if seen[k] < 3}
    assert not short, short


# ---------------------------------------------------------------------------------------------------- the halves, pinned
def _ped(gen, ind, fa, mo):
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)


def _simu(gen, args, pro, anc, states, S, seed):
    """The sample of gen.SimuPlan, checked against the reference with its state and match counts; returns the reference."""
    want = SimuVector(*args, pro, anc, states).sample(S, seed)
    h = gen.SimuPlan(*args, pro, anc, states, simul_no=S, seed=seed)
    try:
        h.compute()
        _same(h.sample_to_host(), want)
        _same(h.state_counts(), state_counts(want))
        sp = np.arange(len(pro)) % 3
        _same(h.match_counts(sp), match_counts(want, sp))
    finally:
        h.close()
    return want


def _ident(gen, args, pro, S, seed):
    want = IdentVector(*args, pro).labels(S, seed)
    h = gen.IdentityPlan(*args, pro, simul_no=S, seed=seed, labels=True)
    try:
        h.compute()
        _same(h.labels_to_host(), want)
        _same(h.counts_to_host(), counts_of(want))
    finally:
        h.close()
    return want


def _link(gen, args, pro, L, q, S, seed):
    want = LinkVector(*args, pro).labels(S, L, q, seed)
    h = gen.SharingPlan(*args, pro, loci=L, q=q, simul_no=S, seed=seed, labels=True)
    try:
        h.compute()
        _same(h.labels_to_host(), want)
        _same(h.sums_to_host(), sums_of(want))
    finally:
        h.close()
    return want


@pytest.mark.gpu
def test_ids_that_differ_only_above_bit_32(gen):
    """Founders 1 and 2; six full sibs 7 + (k << 32), k = 0 .. 5; two more, (9 << 32) + 1 and (9 << 32) + 2; a child of the sibs
    k = 1 and k = 4.  A step kernel that dropped the high half of the ID, or mixed it into the low one, would give the six sibs one
    stream.  On the reference itself: the six sibs' rows are pairwise different, and each row of an ID above 2^32 differs from the
    row its low half alone would draw (the same child of the same couple under the ID & 0xFFFFFFFF; the founders, who draw nothing,
    renamed out of its way)."""
    sibs = [7 + (k << 32) for k in range(6)]
    more = [(9 << 32) + 1, (9 << 32) + 2]
    child = 7 + (6 << 32)
    ind = np.array([1, 2] + sibs + more + [child], dtype=np.int64)
    fa = np.array([0, 0] + [1] * 8 + [sibs[1]], dtype=np.int64)
    mo = np.array([0, 0] + [2] * 8 + [sibs[4]], dtype=np.int64)
    args, seed = (ind, fa, mo), 0x9E3779B97F4A7C15
    pro = np.array(sibs + more + [child, 1], dtype=np.int64)
    high = [k for k, x in enumerate(pro[:8]) if x >> 32]                       # all but the sib k = 0
    assert len(high) == 7

    def low_half_alone(run, *rest):
        """Per proband of `high`, the row of the couple's child under the low half of its ID."""
        rows = {}
        for x in sorted({int(pro[k]) & 0xFFFFFFFF for k in high}):
            a = (np.array([101, 102, x], dtype=np.int64), np.array([0, 0, 101], dtype=np.int64), np.array([0, 0, 102], dtype=np.int64))
            rows[x] = run(a, np.array([x], dtype=np.int64), *rest)[0]
        return [rows[int(pro[k]) & 0xFFFFFFFF] for k in high]

    def conditions(want, cleared):
        for a in range(6):
            for b in range(a):
                assert not np.array_equal(want[a], want[b]), (a, b)
        for k, row in zip(high, cleared):
            assert row.shape == want[k].shape and not np.array_equal(want[k], row), k

    want = _simu(gen, args, pro, [1, 2], [1, 2], 130, seed)
    conditions(want, low_half_alone(lambda a, p: SimuVector(*a, p, [101, 102], [1, 2]).sample(130, seed)))
    want = _ident(gen, args, pro, 130, seed)
    conditions(want, low_half_alone(lambda a, p: IdentVector(*a, p).labels(130, seed)))
    want = _link(gen, args, pro, 129, 0x5555, 3, seed)
    conditions(want, low_half_alone(lambda a, p: LinkVector(*a, p).labels(3, 129, 0x5555, seed)))


@pytest.mark.gpu
def test_seeds_that_differ_only_above_bit_32(gen):
    """The nine individuals of tests/test_link_host.py (an inbred and a selfed child, a half-founder) under the seeds 11,
    11 + 2^32, 11 << 32 and 2^64 - 1: each result equals the reference at its seed, and on the reference no two of the four are
    equal -- a step kernel that dropped the high half of the seed, or put it in the low one's place, would repeat one."""
    from test_link_host import shapes_pedigree
    args = shapes_pedigree()
    pro = np.array([8, 6, 8, 7, 5, 1, 9, 6], dtype=np.int64)
    s = 11
    seeds = [s, s + (1 << 32), s << 32, (1 << 64) - 1]
    runs = (lambda seed: _simu(gen, args, pro, [1, 2, 9], [1, 2, 1], 130, seed), lambda seed: _ident(gen, args, pro, 130, seed),
            lambda seed: _link(gen, args, pro, 129, 0x5555, 3, seed))
    for run in runs:
        want = [run(seed) for seed in seeds]
        for a in range(4):
            for b in range(a):
                assert not np.array_equal(want[a], want[b]), (seeds[a], seeds[b])


@pytest.mark.gpu
def test_fresh_seeds_replay_against_the_reference(gen):
    """seed=None draws 64 fresh bits, so the high half of the key is almost never zero in use: the result of each public function
    equals the reference at the seed it reports (drawn again, at most three times, should the high half come out zero), and a
    second call with that seed returns equal bytes."""
    ped = gen.genealogy(gen.geneaJi)
    args = (ped.ind, ped.father, ped.mother)
    pro, fnd = gen.pro(ped), gen.founder(ped)
    states, sp = np.arange(len(fnd)) % 3, np.arange(len(pro)) % 3

    def fresh(call):
        for _ in range(4):
            r = call(None)
            if r.seed >> 32:
                break
        assert r.seed >> 32 and 0 <= r.seed < 1 << 64
        return r, call(r.seed)

    r, again = fresh(lambda seed: gen.simuProb(ped, pro, sp, fnd, states, simulNo=520, seed=seed))
    want = SimuVector(*args, pro, fnd, states).sample(520, r.seed)
    for x in (r, again):
        assert x.seed == r.seed
        _same(x.marginal, state_counts(want)[np.arange(len(pro)), sp] / 520.0)
        _same(x.by_number, np.bincount(match_counts(want, sp), minlength=len(pro) + 1) / 520.0)
        assert x.joint == x.by_number[-1]
    assert r.marginal.tobytes() == again.marginal.tobytes() and r.by_number.tobytes() == again.by_number.tobytes()

    r, again = fresh(lambda seed: gen.simuIdentity(ped, pro, simulNo=520, seed=seed, labels=True))
    want = IdentVector(*args, pro).labels(520, r.seed)
    for x in (r, again):
        assert x.seed == r.seed
        _same(x.labels, want)
        _same(x.counts, counts_of(want))
    assert r.labels.tobytes() == again.labels.tobytes() and r.counts.tobytes() == again.counts.tobytes()

    r, again = fresh(lambda seed: gen.simuSharing(ped, pro, loci=129, probRecomb=0x5555 / 65536.0, simulNo=5, seed=seed, labels=True))
    assert r.q == 0x5555
    want = LinkVector(*args, pro).labels(5, 129, 0x5555, r.seed)
    for x in (r, again):
        assert x.seed == r.seed
        _same(x.labels, want)
        _same(x.sums, sums_of(want))
    assert r.labels.tobytes() == again.labels.tobytes() and r.sums.tobytes() == again.sums.tobytes()


@pytest.mark.gpu
def test_drop_cases_that_failed_once(gen):
    """Every case of FAILED_ONCE again, with a line here on what was wrong.  (No round has failed a case so far: the list is empty, and
    a loop over it passes where an empty parameter list would report a skipped test.)"""
    for case in FAILED_ONCE:
        what, c = D.run_case(case, gen)
        assert not what, (case, D.describe(c), what)
