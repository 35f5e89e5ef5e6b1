"""Gene dropping without a GPU: the two CPU references of tests/simu_oracle.py against the known answers and each other, the host
plan of gen.SimuPlan (live set, levels, planned positions, argument errors) against the vectorised reference, and gen.descendant /
gen.children against a brute-force set walk."""
import os

import numpy as np
import pytest

from gc_oracle import gc_literal
from occ_oracle import rec_literal
from random_pedigree import random_pedigree
from simu_oracle import KNOWN_ANSWERS, SimuVector, philox_scalar, philox_vector, simu_literal

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "genlib.jl_amd", "data")


def _args(ped):
    return ped.ind, ped.father, ped.mother


def _ped(gen, ind, fa, mo):
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)


def random_case(rng, n):
    """A random pedigree of n individuals with probands (repeats, non-leaves) and ancestors of mixed states anywhere in it."""
    ind, fa, mo, _ = random_pedigree(rng, n, p_founder=0.15, p_one_parent=0.1, p_selfing=0.03, max_back=40)
    pro = rng.choice(ind, size=int(rng.integers(1, 12)), replace=True).astype(np.int64)
    pool = ind[: max(2, n // 2)]
    anc = rng.choice(pool, size=min(int(rng.integers(1, 8)), len(pool)), replace=False).astype(np.int64)
    states = rng.integers(0, 3, size=len(anc)).astype(np.int64)
    return ind, fa, mo, pro, anc, states


def test_philox_known_answers():
    for counter, key, out in KNOWN_ANSWERS:
        assert philox_scalar(counter, key) == out
        assert tuple(int(o) for o in philox_vector(*counter, *key)) == out
    # the three counters at once, as arrays, under each key: row k under key k is the known answer, the others equal the scalar form
    c = np.array([k[0] for k in KNOWN_ANSWERS], dtype=np.uint64)
    for j, (_, key, out) in enumerate(KNOWN_ANSWERS):
        got = np.stack(philox_vector(c[:, 0], c[:, 1], c[:, 2], c[:, 3], *key), axis=1)
        assert got.shape == (3, 4) and tuple(int(o) for o in got[j]) == out
        for k, (counter, _, _) in enumerate(KNOWN_ANSWERS):
            assert tuple(int(o) for o in got[k]) == philox_scalar(counter, key)


def test_oracles_agree_on_geneaJi(gen):
    ped = gen.genealogy(gen.geneaJi)
    pro, fnd = gen.pro(ped), gen.founder(ped)
    states = np.arange(len(fnd)) % 3
    a = simu_literal(*_args(ped), pro, fnd, states, 130, 11)
    b = SimuVector(*_args(ped), pro, fnd, states).sample(130, 11)
    assert a.dtype == b.dtype == np.int8 and np.array_equal(a, b)
    assert len(np.unique(a)) == 3


def test_oracles_agree_on_random_pedigrees():
    rng = np.random.default_rng(2024)
    seen = set()
    for case in range(50):
        n = int(rng.integers(20, 301))
        ind, fa, mo, pro, anc, states = random_case(rng, n)
        seed = int(rng.integers(0, 2**63)) * 2 + case % 2
        a = simu_literal(ind, fa, mo, pro, anc, states, 130, seed)
        b = SimuVector(ind, fa, mo, pro, anc, states).sample(130, seed)
        assert np.array_equal(a, b), case
        seen.update(np.unique(a).tolist())
    assert seen == {0, 1, 2}


def _check_plan(gen, ind, fa, mo, pro, anc, states):
    h = gen.SimuPlan(ind, fa, mo, pro, anc, states, simul_no=64, seed=1)
    try:
        o = SimuVector(ind, fa, mo, pro, anc, states)
        assert (h.n_live, h.levels) == (o.n_live, o.levels)
        assert np.array_equal(h.rows_per_level(), o.rows_per_level)
        r = h.rows()
        # rows are the live individuals ordered by level; the parent rows name the live parents
        pos = {int(x): k for k, x in enumerate(np.asarray(ind).tolist())}
        at = np.array([pos[int(x)] for x in r["ids"]], dtype=np.int64)
        assert np.array_equal(np.sort(at), np.flatnonzero(o.level >= 0))
        assert np.all(np.diff(o.level[at]) >= 0)
        row_of = np.full(len(ind), -1, dtype=np.int64)
        row_of[at] = np.arange(len(at))
        for parent, got in ((o.fa, r["father_rows"]), (o.mo, r["mother_rows"])):
            q = parent[at]
            want = np.where((q >= 0) & (o.level[at] > 0), row_of[np.maximum(q, 0)], -1)
            assert np.array_equal(got, want)
        want = np.where(o.state[o.pro] >= 0, -2 - o.state[o.pro], row_of[o.pro])
        assert np.array_equal(r["pro_positions"], want)
        return h.n_live, r
    finally:
        h.close()


@pytest.mark.parametrize("name", ["geneaJi.csv", "genea140.csv"])
def test_plan_matches_oracle_on_bundled_pedigrees(gen, name):
    ped = gen.genealogy(os.path.join(DATA, name))
    fnd = gen.founder(ped)
    n_live, _ = _check_plan(gen, *_args(ped), gen.pro(ped), fnd, np.arange(len(fnd)) % 3)
    assert n_live > 0
    _check_plan(gen, *_args(ped), gen.pro(ped)[:3], fnd[:5], [1, 0, 2, 1, 1])


def test_plan_matches_oracle_on_random_pedigrees(gen):
    rng = np.random.default_rng(99)
    live = 0
    for _ in range(200):
        ind, fa, mo, pro, anc, states = random_case(rng, int(rng.integers(5, 400)))
        live += _check_plan(gen, ind, fa, mo, pro, anc, states)[0]
    assert live > 1000


def shapes_pedigree():
    """1, 2 founders; 3 = (1, 2); 4 founder; 5 = (3, 4); 6 = (5, 0); 7 founder; 8 = (7, 0); 9 = (6, 8); 10 = (0, 8)."""
    ind = np.arange(1, 11, dtype=np.int64)
    fa = np.array([0, 0, 1, 0, 3, 5, 0, 7, 6, 0], dtype=np.int64)
    mo = np.array([0, 0, 2, 0, 4, 0, 0, 0, 8, 8], dtype=np.int64)
    return ind, fa, mo


def test_planned_positions():
    import genlib_jl_amd as gen
    ind, fa, mo = shapes_pedigree()
    # ancestors 1 (state 1) and 3 (state 2, below 1: it ignores 1); probands: 9 (live), 10 (outside L), 3 (a listed ancestor), 9 again.
    # 1 is a carrier and an ancestor of the proband 3: it has its row, and nobody reads it
    n_live, r = _check_plan(gen, ind, fa, mo, [9, 10, 3, 9], [1, 3], [1, 2])
    assert r["ids"].tolist() == [1, 3, 5, 6, 9] and n_live == 5
    assert r["pro_positions"].tolist() == [4, -1, -4, 4]
    assert r["father_rows"].tolist() == [-1, -1, 1, 2, 3] and r["mother_rows"].tolist() == [-1] * 5
    # a state-0 blocker: 5 listed with state 0 cuts 9 off from 1; 8's line is not marked at all
    n_live, r = _check_plan(gen, ind, fa, mo, [9, 5], [1, 5], [2, 0])
    assert n_live == 2 and r["ids"].tolist() == [1, 3] and r["pro_positions"].tolist() == [-1, -2]
    # the same blocker with the second line marked: 9 is live through its mother only, its father 6 is a zero row
    n_live, r = _check_plan(gen, ind, fa, mo, [9], [1, 5, 7], [2, 0, 1])
    assert r["ids"].tolist() == [1, 7, 3, 8, 9]
    assert r["father_rows"].tolist() == [-1, -1, 0, 1, -1] and r["mother_rows"].tolist() == [-1, -1, -1, -1, 3]


def test_argument_errors(gen):
    ind, fa, mo = shapes_pedigree()
    ok = dict(pro_ids=[9], anc_ids=[1, 7], anc_states=[1, 2], simul_no=10, seed=3)

    def plan(**kw):
        gen.SimuPlan(ind, fa, mo, **{**ok, **kw}).close()

    plan()
    plan(anc_ids=[1, 7, 1], anc_states=[1, 2, 1])                       # an equal repeat is allowed
    plan(simul_no=1 << 24)
    for kw in (dict(pro_ids=[99]), dict(anc_ids=[1, 99])):
        with pytest.raises(KeyError):
            plan(**kw)
    for kw in (dict(anc_states=[1, 3]), dict(anc_states=[-1, 1]), dict(anc_states=[1]), dict(anc_states=[1, 2, 1]),
               dict(anc_ids=[1, 7, 1], anc_states=[1, 2, 2]), dict(simul_no=0), dict(simul_no=(1 << 24) + 1), dict(pro_ids=[]),
               dict(anc_ids=[], anc_states=[])):
        with pytest.raises(ValueError):
            plan(**kw)
    ped = _ped(gen, ind, fa, mo)
    with pytest.raises(TypeError):
        gen.simuSample(ped, probRecomb=(0.0, 0.0))
    with pytest.raises(TypeError):
        gen.simuProb(ped, [9], [1], [1], [1], probSurvival=1.0)
    with pytest.raises(ValueError):
        gen.simuProb(ped, [9], [3], [1], [1])
    with pytest.raises(ValueError):
        gen.simuProb(ped, [9], [1, 1], [1], [1])
    h = gen.SimuPlan(ind, fa, mo, [9], [1], [1], seed=None)
    h2 = gen.SimuPlan(ind, fa, mo, [9], [1], [1], seed=None)
    assert 0 <= h.seed < 2**64 and h.seed != h2.seed and h.simul_no == 5000
    h.close()
    h2.close()


def _brute_children(ind, fa, mo):
    kids = {int(x): set() for x in ind}
    for x, f, m in zip(ind.tolist(), fa.tolist(), mo.tolist()):
        for q in (f, m):
            if q:
                kids[q].add(x)
    return kids


def _brute_descendants(kids, ids):
    out, todo = set(), list(ids)
    while todo:
        for c in kids[todo.pop()]:
            if c not in out:
                out.add(c)
                todo.append(c)
    return sorted(out)


def _check_descent(gen, ped, ids):
    kids = _brute_children(ped.ind, ped.father, ped.mother)
    for x in ids:
        x = int(x)
        got = gen.children(ped, x)
        assert got.dtype == np.int64 and got.tolist() == sorted(kids[x])
        got = gen.descendant(ped, x)
        assert got.dtype == np.int64 and got.tolist() == _brute_descendants(kids, [x])
    ids = [int(x) for x in ids]
    assert gen.descendant(ped, ids).tolist() == _brute_descendants(kids, ids)
    assert gen.descendant(ped, np.asarray(ids[:2])).tolist() == _brute_descendants(kids, ids[:2])


def test_descendant_and_children(gen):
    ji = gen.genealogy(gen.geneaJi)
    _check_descent(gen, ji, ji.ind)
    g140 = gen.genealogy(gen.genea140)
    rng = np.random.default_rng(5)
    _check_descent(gen, g140, np.concatenate([gen.founder(g140)[:10], rng.choice(g140.ind, size=10, replace=False)]))
    for _ in range(20):
        ind, fa, mo, _ = random_pedigree(rng, int(rng.integers(2, 200)), 0.2, 0.1, 0.05, 30)
        _check_descent(gen, _ped(gen, ind, fa, mo), rng.choice(ind, size=min(len(ind), 8), replace=False))
    for ped in (ji, g140):
        with pytest.raises(KeyError):
            gen.descendant(ped, 10**9)
        with pytest.raises(KeyError):
            gen.descendant(ped, [int(ped.ind[0]), 10**9])
        with pytest.raises(KeyError):
            gen.children(ped, 10**9)
    assert gen.children(ji, int(gen.pro(ji)[0])).tolist() == [] and gen.descendant(ji, int(gen.pro(ji)[0])).tolist() == []


def test_descendants_cover_what_rec_counts(gen):
    """gen.rec's notion of coverage where both apply (strict descendants, distinct probands): the probands among a founder's
    descendants are as many as tests/occ_oracle.py's rec_literal counts (gen.rec itself: tests/test_simu_gpu.py), and they are the
    live probands of a plan with that founder alone."""
    for ped in (gen.genealogy(gen.geneaJi), gen.genealogy(gen.genea140)):
        pro = gen.pro(ped)
        fnd = gen.founder(ped)[:6]
        rec = rec_literal(*_args(ped), pro, fnd)
        assert rec.any()
        for f, n in zip(fnd, rec):
            covered = np.intersect1d(gen.descendant(ped, int(f)), pro)
            assert len(covered) == n
            h = gen.SimuPlan(*_args(ped), pro, [f], [1], simul_no=1, seed=0)
            try:
                assert np.array_equal(pro[h.rows()["pro_positions"] >= 0], covered)
            finally:
                h.close()


def test_oracle_mean_meets_gc_on_geneaJi(gen):
    """One condition, not a measurement.  With one founder as the only ancestor, state 1, the expected count of a proband is its
    genetic contribution (every path of d meioses passes the one marked copy on with probability 2^-d).  A count has variance
    <= 1, so 1 / sqrt(S) bounds the standard deviation of the mean of S simulations; the margin is 5 of them."""
    ped = gen.genealogy(gen.geneaJi)
    pro, S = gen.pro(ped), 5000
    for f in gen.founder(ped)[:6]:
        mean = SimuVector(*_args(ped), pro, [f], [1]).sample(S, 7).mean(axis=1, dtype=np.float64)
        want = gc_literal(*_args(ped), pro, [f])[:, 0].astype(np.float64)
        dev = np.abs(mean - want).max() * np.sqrt(S)
        print("founder %d: largest deviation %.3f / sqrt(S)" % (int(f), dev))
        assert dev <= 5.0
