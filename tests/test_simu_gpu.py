"""Gene dropping on the MI355X (gen.SimuPlan, gen.simuSample, gen.simuProb) against the vectorised reference of
tests/simu_oracle.py: every comparison is np.array_equal, every handle is computed twice with equal bits.  Shapes are the smallest
at which each part of csrc/simu.hip can go wrong: word and pair edges of the simulations, every lanes-per-row form of the step
kernel (pinned through stats()), forced and ragged panels, long child lists, deep chains, blockers, the plane limit of the match
kernel."""
import numpy as np
import pytest

from random_pedigree import random_pedigree
from simu_oracle import SimuVector, match_counts, state_counts

pytestmark = pytest.mark.gpu

EDGES = [1, 63, 64, 65, 127, 128, 129, 5000]


def _args(ped):
    return ped.ind, ped.father, ped.mother


def _ped(gen, ind, fa, mo):
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b), np.argwhere(a != b)[:5]


def _check(gen, args, pro, anc, states, S, seed, want=None, no_sample=False, rng=None):
    """Sample, state counts and match counts (a random statePro, asked twice, then another) of one handle, computed twice, against
    the reference; returns (stats, reference sample)."""
    if want is None:
        want = SimuVector(*args, pro, anc, states).sample(S, seed)
    rng = np.random.default_rng(S + len(pro)) if rng is None else rng
    h = gen.SimuPlan(*args, pro, anc, states, simul_no=S, seed=seed, no_sample=no_sample)
    try:
        for _ in range(2):
            h.compute()
            if no_sample:
                with pytest.raises(ValueError):
                    h.sample_to_host()
            else:
                _same(h.sample_to_host(), want)
            _same(h.state_counts(), state_counts(want))
            for k in range(2):
                sp = rng.integers(0, 3, size=len(pro))
                _same(h.match_counts(sp), match_counts(want, sp))
                _same(h.match_counts(sp), match_counts(want, sp))
            _same(h.state_counts(), state_counts(want))
        return h.stats(), want
    finally:
        h.close()


@pytest.fixture(scope="module")
def ji(gen):
    ped = gen.genealogy(gen.geneaJi)
    fnd = gen.founder(ped)
    return ped, gen.pro(ped), fnd, np.arange(len(fnd)) % 3


@pytest.fixture(scope="module")
def big(gen):
    """2,000 individuals with founders anywhere, one-parent members and selfing (the recipe of test_implex_gpu.py's word_edge_case);
    129 probands with repeats and non-leaves, 60 ancestors of mixed states in the older half (some below others)."""
    rng = np.random.default_rng(77)
    ind, fa, mo, _ = random_pedigree(rng, 2000, p_founder=0.08, p_one_parent=0.1, p_selfing=0.02, max_back=300, max_depth=14)
    pro = rng.choice(ind[600:], size=129, replace=True).astype(np.int64)
    pro[64], pro[128] = pro[0], pro[5]
    anc = rng.choice(ind[:900], size=60, replace=False).astype(np.int64)
    states = rng.integers(0, 3, size=60).astype(np.int64)
    pro[7] = anc[np.flatnonzero(states == 2)[0]]                        # a proband that is a listed ancestor
    return _ped(gen, ind, fa, mo), pro, anc, states


@pytest.mark.parametrize("S", EDGES)
def test_word_and_pair_edges(gen, ji, big, S):
    for ped, pro, anc, states in (ji, big):
        stats, want = _check(gen, _args(ped), pro, anc, states, S, 2024)
        assert stats["panels"] == 1 and stats["panel_cols"] == (S + 127) // 128 * 128 and stats["n_live"] > 0
    assert len(np.unique(want)) == 3 or S == 1


@pytest.mark.parametrize("S", [16, 80, 144, 4112])
def test_sample_rows_on_16_bytes_with_a_partial_last_word(gen, ji, big, S):
    """S a multiple of 16 but not of 64: the full words of a row go out as 16-byte stores, the last word byte by byte."""
    for ped, pro, anc, states in (ji, big):
        _check(gen, _args(ped), pro, anc, states, S, 77)


def test_big_case_has_the_shapes_it_claims(gen, big):
    ped, pro, anc, states = big
    o = SimuVector(*_args(ped), pro, anc, states)
    assert o.levels >= 5 and o.n_live >= 200
    assert np.any(o.level[o.pro] < 0) and np.any(o.state[o.pro] == 2)              # a proband outside L, one that is an ancestor
    listed = np.flatnonzero(o.state >= 0)
    anc_of = gen.ancestor(ped, ped.ind[listed])
    assert np.intersect1d(anc_of, ped.ind[listed]).size > 0                        # a listed ancestor below another
    fa, mo = o.fa, o.mo
    assert np.any((fa >= 0) & (fa == mo) & (o.level > 0)) and np.any(((fa < 0) != (mo < 0)) & (o.level > 0))   # selfing, one parent


@pytest.mark.parametrize("pairs", [1, 2, 4, 8, 16, 32, 64, 65, 3])
def test_every_lanes_per_row_form(gen, ji, pairs):
    ped, pro, anc, states = ji
    S = 128 * pairs - (5 if pairs == 3 else 0)
    stats, _ = _check(gen, _args(ped), pro, anc, states, S, 5)
    want = 1
    while want < pairs and want < 64:
        want *= 2
    assert stats["lanes_per_row"] == want and stats["panel_cols"] == 128 * pairs and stats["panels"] == 1
    o = SimuVector(*_args(ped), pro, anc, states)
    assert stats["n_live"] == o.n_live and stats["levels"] == o.levels
    assert stats["algorithmic_bytes"] == 3 * 32 * pairs * (o.n_live - o.rows_per_level[0])


@pytest.mark.parametrize("no_sample", [False, True])
def test_forced_panels(gen, big, monkeypatch, no_sample):
    ped, pro, anc, states = big
    S = 5000
    want = SimuVector(*_args(ped), pro, anc, states).sample(S, 9)
    for env, cols, panels in (("128", 128, 40), ("1000", 1024, 5), ("5000", 5120, 1), ("100000", 5120, 1)):
        monkeypatch.setenv("GENPHI_SIMU_PANEL", env)
        stats, _ = _check(gen, _args(ped), pro, anc, states, S, 9, want=want, no_sample=no_sample)
        assert (stats["panel_cols"], stats["panels"]) == (cols, panels)
    monkeypatch.delenv("GENPHI_SIMU_PANEL")
    stats, _ = _check(gen, _args(ped), pro, anc, states, S, 9, want=want, no_sample=no_sample)
    assert (stats["panel_cols"], stats["panels"]) == (5120, 1)


def _hub(n_children):
    ind = np.arange(1, n_children + 3, dtype=np.int64)
    fa = np.where(ind > 2, 1, 0).astype(np.int64)
    mo = np.where(ind > 2, 2, 0).astype(np.int64)
    return ind, fa, mo


def test_hub_couple_with_300_children(gen):
    ind, fa, mo = _hub(300)
    stats, want = _check(gen, (ind, fa, mo), ind[2:], [1, 2], [1, 2], 200, 3)
    assert stats["levels"] == 2 and stats["n_live"] == 302
    assert np.all(want >= 1) and len(np.unique(want[:, :64], axis=0)) > 100        # the mother always gives one; children differ


@pytest.mark.parametrize("n_pro", [255, 256, 257, 600])
def test_match_plane_limit(gen, n_pro):
    """255, 256 and 257 probands around the width of a plane set.  At S = 130 a row has 4 words, a block 64 groups, and a group walks
    only a few of them: these cases check the dealing of probands to groups and the three match words.  The limit itself, groups
    that walk 255 probands with every plane full, is pinned by test_match_full_planes_and_two_blocks below."""
    ind, fa, mo = _hub(600)
    pro = ind[2:2 + n_pro]
    for sp in (np.ones(n_pro, dtype=np.int64), np.full(n_pro, 2), np.zeros(n_pro, dtype=np.int64)):
        st = [2, 2] if sp[0] == 2 else ([1, 0] if sp[0] == 1 else [0, 1])
        h = gen.SimuPlan(ind, fa, mo, pro, [1, 2], st, simul_no=130, seed=1)
        try:
            h.compute()
            got = h.match_counts(sp)
            _same(got, match_counts(SimuVector(ind, fa, mo, pro, [1, 2], st).sample(130, 1), sp))
            if sp[0] == 2:
                assert np.all(got == n_pro)                                      # every proband matches in every simulation
        finally:
            h.close()
    # no live row at all: state 0 everywhere
    h = gen.SimuPlan(ind, fa, mo, pro, [1, 2], [0, 0], simul_no=130, seed=1)
    try:
        h.compute()
        assert h.n_live == 0 and np.all(h.match_counts(np.zeros(n_pro, dtype=np.int64)) == n_pro) and not h.sample_to_host().any()
        _same(h.state_counts(), np.tile(np.array([130, 0, 0], dtype=np.int64), (n_pro, 1)))
    finally:
        h.close()


def test_match_full_planes_and_two_blocks(gen):
    """The test that pins the 255-row plane limit of the match kernel.  64 words per row: 4 groups per block walk 255 probands each (every plane full where all match), the 1,021st proband is
    the second block's."""
    ind, fa, mo = _hub(1021)
    pro = ind[2:]
    h = gen.SimuPlan(ind, fa, mo, pro, [1, 2], [2, 1], simul_no=4096, seed=6, no_sample=True)
    try:
        h.compute()
        got = h.match_counts(np.full(1021, 2))
        want = SimuVector(ind, fa, mo, pro, [1, 2], [2, 1]).sample(4096, 6)
        _same(got, match_counts(want, np.full(1021, 2)))
        assert np.all(h.match_counts(np.zeros(1021, dtype=np.int64)) == 0)           # the father always gives one
        _same(h.match_counts(np.arange(1021) % 3), match_counts(want, np.arange(1021) % 3))
    finally:
        h.close()
    h = gen.SimuPlan(ind, fa, mo, pro, [1, 2], [2, 2], simul_no=4096, seed=6, no_sample=True)
    try:
        h.compute()
        assert np.all(h.match_counts(np.full(1021, 2)) == 1021)
    finally:
        h.close()


def test_chain_of_300_levels(gen):
    n = 300
    ind = np.arange(1, 2 * n, dtype=np.int64)            # 1; then (mate, child) pairs: child k = (previous child, mate)
    fa, mo = np.zeros(2 * n - 1, dtype=np.int64), np.zeros(2 * n - 1, dtype=np.int64)
    prev = 1
    for k in range(1, n):
        mate, child = 2 * k, 2 * k + 1
        fa[child - 1], mo[child - 1] = (prev, mate) if k % 2 else (mate, prev)
        prev = child
    pro = np.array([3, 5, 21, 2 * n - 1, 2], dtype=np.int64)
    stats, want = _check(gen, (ind, fa, mo), pro, [1], [2], 5000, 8)
    assert stats["levels"] == n and stats["n_live"] == n
    assert np.all(want[0] == 1) and 0.4 < want[1].mean() < 0.6 and want[2].mean() < 0.05 and not want[3].any() and not want[4].any()


def test_shapes_blockers_and_mixed_states(gen):
    from test_simu_host import shapes_pedigree
    ind, fa, mo = shapes_pedigree()
    args = (ind, fa, mo)
    S = 300
    # a proband that is a listed ancestor (its state in every simulation), one outside L (zeros), duplicated probands (equal rows),
    # a listed ancestor below another
    _, want = _check(gen, args, [9, 10, 3, 9, 1], [1, 3], [1, 2], S, 4)
    assert np.all(want[2] == 2) and np.all(want[4] == 1) and not want[1].any() and np.array_equal(want[0], want[3]) and want[0].any()
    # a state-0 blocker cuts the only marked line
    _, want = _check(gen, args, [9, 5, 3], [1, 5], [2, 0], S, 4)
    assert not want[0].any() and not want[1].any() and np.all(want[2] == 1)
    # states 0 / 1 / 2 mixed, one-parent members on both lines
    _, want = _check(gen, args, [9, 10, 6, 8], [1, 5, 7, 2], [2, 0, 1, 1], S, 4)
    assert not want[2].any() and want[0].any() and want[1].any() and want[0].max() == 1
    # selfing: both sides draw their own words
    ind2 = np.array([1, 2, 3], dtype=np.int64)
    _, want = _check(gen, (ind2, np.array([0, 1, 2]), np.array([0, 1, 2])), [2, 3], [1], [1], 2000, 4)
    assert set(np.unique(want[0]).tolist()) == {0, 1, 2} and abs((want[0] == 1).mean() - 0.5) < 0.06


def test_invariants(gen, big):
    ped, pro, anc, states = big
    full = gen.simuSample(ped, pro, anc, states, simulNo=5000, seed=31)
    assert full.dtype == np.int8 and full.shape == (len(pro), 5000)
    _same(gen.simuSample(ped, pro, anc, states, simulNo=64, seed=31), np.ascontiguousarray(full[:, :64]))
    _same(gen.simuSample(ped, pro, anc, states, simulNo=129, seed=31), np.ascontiguousarray(full[:, :129]))
    sub = np.array([100, 3, 3, 64, 7])
    _same(gen.simuSample(ped, pro[sub], anc, states, simulNo=5000, seed=31), full[sub])
    # gen.branching keeps the individuals between the probands and the ancestors: a proband that descends from no listed ancestor
    # leaves the pedigree (its rows are zero), and so does an ancestor without a listed proband below it (it marks no row);
    # every other row is unchanged
    pruned = gen.branching(ped, pro=pro, ancestors=anc)
    kept = np.array([int(p) in pruned for p in pro])
    akept = np.array([int(a) in pruned for a in anc])
    assert len(pruned) < len(ped) and kept.sum() > 50 and not kept.all() and not full[~kept].any() and akept.sum() > 20
    _same(gen.simuSample(pruned, pro[kept], anc[akept], states[akept], simulNo=5000, seed=31), full[kept])
    other = gen.simuSample(ped, pro, anc, states, simulNo=5000, seed=32)
    assert not np.array_equal(other, full)
    a, b = gen.simuSample(ped, pro, anc, states, simulNo=256), gen.simuSample(ped, pro, anc, states, simulNo=256)
    assert not np.array_equal(a, b)                                              # fresh seeds
    # defaults: pro(ped), founder(ped), all states 1
    dflt = gen.simuSample(ped, simulNo=130, seed=1)
    _same(dflt, SimuVector(*_args(ped), gen.pro(ped), gen.founder(ped), np.ones(len(gen.founder(ped)))).sample(130, 1))


def test_descendants_cover_what_gen_rec_counts(gen):
    """gen.rec's notion of coverage where both apply (strict descendants, distinct probands): gen.descendant(ped, founder) has as
    many of pro(ped) as gen.rec counts, and they are the probands with a live row in a plan with that founder alone."""
    for ped in (gen.genealogy(gen.geneaJi), gen.genealogy(gen.genea140)):
        pro, fnd = gen.pro(ped), gen.founder(ped)[:40]
        rec = gen.rec(ped, pro, fnd)
        assert rec.any()
        for f, n in zip(fnd.tolist(), rec.tolist()):
            assert len(np.intersect1d(gen.descendant(ped, f), pro)) == n
        for f in fnd[:6].tolist():
            h = gen.SimuPlan(*_args(ped), pro, [f], [1], simul_no=1, seed=0)
            try:
                assert np.array_equal(pro[h.rows()["pro_positions"] >= 0], np.intersect1d(gen.descendant(ped, f), pro))
            finally:
                h.close()


def test_simuProb(gen, big):
    ped, pro, anc, states = big
    pro = pro[:40]
    S, seed = 5000, 12
    want = SimuVector(*_args(ped), pro, anc, states).sample(S, seed)
    rng = np.random.default_rng(1)
    for sp in (rng.integers(0, 3, size=len(pro)), np.zeros(len(pro), dtype=np.int64), want[:, 17].astype(np.int64)):
        r = gen.simuProb(ped, pro, sp, anc, states, simulNo=S, seed=seed)
        assert (r.simulNo, r.seed) == (S, seed) and isinstance(r.joint, float)
        _same(r.marginal, state_counts(want)[np.arange(len(pro)), sp] / float(S))
        _same(r.by_number, np.bincount(match_counts(want, sp), minlength=len(pro) + 1) / float(S))
        assert r.by_number.shape == (len(pro) + 1,) and abs(r.by_number.sum() - 1.0) <= (len(pro) + 1) * 2.0 ** -53
        assert r.joint == r.by_number[-1]
    assert r.joint >= 1.0 / S                                                    # simulation 17 matches itself
    assert gen.simuProb(ped, pro, sp, anc, states, simulNo=S).seed != gen.simuProb(ped, pro, sp, anc, states, simulNo=S).seed


def test_mean_count_meets_gc_on_genea140(gen):
    """One condition, not a measurement: with one founder as the only ancestor, state 1, the mean count of every proband over S
    simulations lies within 5 / sqrt(S) of gen.gc (a count has variance <= 1: 1 / sqrt(S) bounds the standard deviation of the
    mean).  The founders: the first three with a live proband; the reference meets the condition for them."""
    ped = gen.genealogy(gen.genea140)
    pro, S = gen.pro(ped), 5000
    assert len(pro) == 140
    picked = []
    for f in gen.founder(ped):
        if np.intersect1d(gen.descendant(ped, int(f)), pro).size:
            picked.append(int(f))
        if len(picked) == 3:
            break
    for f in picked:
        gc = gen.gc(ped, pro, [f])[:, 0].astype(np.float64)
        assert gc.any()
        ref = SimuVector(*_args(ped), pro, [f], [1]).sample(S, 7)
        got = gen.simuSample(ped, pro, [f], [1], simulNo=S, seed=7)
        _same(got, ref)
        for name, sample in (("reference", ref), ("device", got)):
            dev = np.abs(sample.mean(axis=1, dtype=np.float64) - gc).max() * np.sqrt(S)
            print("founder %d, %s: largest deviation %.3f / sqrt(S)" % (f, name, dev))
            assert dev <= 5.0
