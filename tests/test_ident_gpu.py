"""gen.simuIdentity on the MI355X (gen.IdentityPlan, gen.simuIdentity) against the vectorised reference of tests/ident_oracle.py:
every comparison is np.array_equal, for the counts and, with the flag, the labels; every handle is computed twice with equal bytes.
Shapes are the smallest at which each part of csrc/ident.hip can go wrong: word and pair edges of the simulations, forced and
ragged panels, allele tables at the plane edges, probands at the pair kernel's tile edges (the tile is read from stats()), every
lanes-per-row form of the step kernel, long child lists, deep chains, half-founders, selfing and repeats.  A reference is computed
once per pedigree at the largest S and cut to the columns a case needs (the prefix rule of the definition, checked on the
reference itself in tests/test_ident_host.py)."""
import numpy as np
import pytest

from exact_kinship import ExactKinship
from ident_oracle import IdentVector, counts_of, swap_roles
from random_pedigree import random_pedigree

pytestmark = pytest.mark.gpu

EDGES = [1, 63, 64, 65, 127, 128, 129, 200, 5000]


def _args(ped):
    return ped.ind, ped.father, ped.mother


def _ped(gen, ind, fa, mo):
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b), np.argwhere(a != b)[:5]


def _check(gen, args, pro, S, seed, want=None, labels=True, **kw):
    """Counts and labels of one handle, computed twice, against the reference labels want (n_pro, 2, >= S); returns stats()."""
    if want is None:
        want = IdentVector(*args, pro).labels(S, seed)
    want = np.ascontiguousarray(want[:, :, :S])
    counts = counts_of(want)
    h = gen.IdentityPlan(*args, pro, simul_no=S, seed=seed, labels=labels, **kw)
    try:
        for _ in range(2):
            h.compute()
            _same(h.counts_to_host(), counts)
            if labels:
                _same(h.labels_to_host(), want)
            else:
                with pytest.raises(ValueError):
                    h.labels_to_host()
        st = h.stats()
        assert st["sweep_ms"] >= 0.0 and st["pair_ms"] > 0.0 and st["algorithmic_bytes"] >= 0.0
        n = len(pro)
        pairs = n * n if kw.get("all_pairs") else n * (n + 1) // 2
        assert st["word_ops"] == pairs * ((S + 63) // 64) * (12 * h.planes + 40) and st["planes"] == h.planes
        return st
    finally:
        h.close()


@pytest.fixture(scope="module")
def ji(gen):
    ped = gen.genealogy(gen.geneaJi)
    pro = gen.pro(ped)
    return ped, pro, IdentVector(*_args(ped), pro).labels(128 * 65, 2024)


@pytest.fixture(scope="module")
def big(gen):
    """600 individuals with founders anywhere, half-founders and selfing; 40 probands (two tiles) with repeats, non-leaves and a
    founder; the reference labels at S = 5000."""
    rng = np.random.default_rng(77)
    ind, fa, mo, _ = random_pedigree(rng, 600, p_founder=0.08, p_one_parent=0.1, p_selfing=0.03, max_back=60, max_depth=14)
    pro = rng.choice(ind[200:], size=40, replace=False).astype(np.int64)
    pro[33], pro[17], pro[5] = pro[0], pro[0], ind[0]
    return (ind, fa, mo), pro, IdentVector(ind, fa, mo, pro).labels(5000, 9)


@pytest.mark.parametrize("S", EDGES)
def test_word_and_pair_edges(gen, ji, S):
    ped, pro, want = ji
    st = _check(gen, _args(ped), pro, S, 2024, want=want)
    assert st["panels"] == 1 and st["panel_cols"] == (S + 127) // 128 * 128
    if S == 5000:
        assert np.all(counts_of(want[:, :, :S]).sum(axis=(0, 1)) > 0)                 # all nine states occur among the three probands


def test_big_case_has_the_shapes_it_claims(big):
    (ind, fa, mo), pro, want = big
    o = IdentVector(ind, fa, mo, pro)
    assert o.levels >= 5 and o.n_live >= 150 and o.planes >= 6
    lf, lm = o.fa[o.live], o.mo[o.live]
    assert np.any((lf >= 0) & (lf == lm)) and np.any((lf < 0) != (lm < 0))               # selfing, half-founders
    c = counts_of(want)
    assert np.all(c.sum(axis=(0, 1)) > 0) and np.array_equal(swap_roles(c), c)


@pytest.mark.parametrize("all_pairs", [False, True])
def test_forced_panels(gen, big, all_pairs):
    args, pro, want = big
    for cols, panel_cols, panels in ((128, 128, 40), (1000, 1024, 5), (5000, 5120, 1), (100000, 5120, 1), (0, 5120, 1)):
        st = _check(gen, args, pro, 5000, 9, want=want, labels=cols != 128, panel_cols=cols, all_pairs=all_pairs)
        assert (st["panel_cols"], st["panels"]) == (panel_cols, panels)
    assert (st["tile_rows"], st["tile_cols"]) == (32, 32) and len(pro) > st["tile_rows"]


def _founders_and_sibships(n_founders, half_founder):
    """n_founders unrelated founders, three children of founders 1 and 2 (of founder 1 selfed when it is alone), and on request a
    half-founder child of founder 1 with an inbred child of its own; everyone is a proband."""
    ind = list(range(1, n_founders + 1))
    fa, mo = [0] * n_founders, [0] * n_founders
    mate = 2 if n_founders >= 2 else 1
    for _ in range(3):
        ind.append(len(ind) + 1)
        fa.append(1)
        mo.append(mate)
    if half_founder:
        ind += [len(ind) + 1, len(ind) + 2]
        fa += [1, ind[-2]]
        mo += [0, n_founders + 1]
    return np.array(ind, dtype=np.int64), np.array(fa, dtype=np.int64), np.array(mo, dtype=np.int64)


@pytest.mark.parametrize("n_founders,half,n_labels,planes", [(1, False, 2, 1), (1, True, 3, 2), (2, False, 4, 2), (2, True, 5, 3),
                                                           (128, False, 256, 8), (128, True, 257, 9)])
def test_allele_tables_at_the_plane_edges(gen, n_founders, half, n_labels, planes):
    """B = 1, 2, 3, 8 and 9 around the powers of two.  (n_labels = 1 cannot occur: a live set has an individual without parents,
    who carries two founder alleles.)"""
    ind, fa, mo = _founders_and_sibships(n_founders, half)
    h = gen.IdentityPlan(ind, fa, mo, ind, simul_no=200, seed=3)
    assert (h.n_labels, h.planes) == (n_labels, planes)
    h.close()
    st = _check(gen, (ind, fa, mo), ind, 200, 3)
    assert st["planes"] == planes


@pytest.fixture(scope="module")
def clan():
    """120 individuals in few generations, closely related: the pool the tile-edge cases draw their probands from."""
    rng = np.random.default_rng(3)
    ind, fa, mo, _ = random_pedigree(rng, 120, p_founder=0.1, p_one_parent=0.05, p_selfing=0.05, max_back=20)
    return (ind, fa, mo), rng.permutation(ind)


@pytest.mark.parametrize("edge", ["one", "tile - 1", "tile", "tile + 1", "two tiles + 1", "three tiles + 3"])
def test_probands_at_the_tile_edges(gen, clan, edge):
    args, order = clan
    h = gen.IdentityPlan(*args, order[:1], simul_no=1, seed=0)
    tile = h.stats()["tile_rows"]
    assert tile == h.stats()["tile_cols"]
    h.close()
    n = {"one": 1, "tile - 1": tile - 1, "tile": tile, "tile + 1": tile + 1, "two tiles + 1": 2 * tile + 1, "three tiles + 3": 3 * tile + 3}[edge]
    pro = order[:n]
    # (the labels of a sub-list are named by its own allele table: the reference is asked again, the simulation is the same)
    want = IdentVector(*args, pro).labels(200, 5)
    for all_pairs in (False, True):
        _check(gen, args, pro, 200, 5, want=want, all_pairs=all_pairs, labels=not all_pairs)
    # the two tiles + 1 rows and columns in both directions: rows and columns are the same list, the transposed array says so
    if edge == "two tiles + 1":
        c = counts_of(want)
        assert np.array_equal(swap_roles(c), c) and c.shape == (2 * tile + 1,) * 2 + (9,)


@pytest.mark.parametrize("pairs", [1, 2, 4, 8, 16, 32, 64, 65, 3])
def test_every_lanes_per_row_form(gen, ji, pairs):
    ped, pro, want = ji
    S = 128 * pairs - (5 if pairs == 3 else 0)
    st = _check(gen, _args(ped), pro, S, 2024, want=want)
    lpr = 1
    while lpr < pairs and lpr < 64:
        lpr *= 2
    assert st["lanes_per_row"] == lpr and st["panel_cols"] == 128 * pairs and st["panels"] == 1
    o = IdentVector(*_args(ped), pro)
    assert st["levels"] == o.levels and st["algorithmic_bytes"] == 48 * o.planes * (2 * o.n_live - o.n_labels) * pairs


def test_hub_couple_with_300_children(gen):
    ind = np.arange(1, 303, dtype=np.int64)
    fa = np.where(ind > 2, 1, 0).astype(np.int64)
    mo = np.where(ind > 2, 2, 0).astype(np.int64)
    want = IdentVector(ind, fa, mo, ind).labels(200, 3)
    st = _check(gen, (ind, fa, mo), ind, 200, 3, want=want)
    assert st["levels"] == 2 and st["planes"] == 2
    c = counts_of(want)
    assert np.all(c[2:, 2:, :6] == 0) and np.all(c[2:, 2:, 6:].sum(axis=(0, 1)) > 0)      # sibs of unrelated parents: states 7, 8, 9


def test_chain_of_300_levels(gen):
    n = 300
    ind = np.arange(1, 2 * n, dtype=np.int64)            # 1; then (mate, child) pairs: child k = (previous child, mate)
    fa, mo = np.zeros(2 * n - 1, dtype=np.int64), np.zeros(2 * n - 1, dtype=np.int64)
    prev = 1
    for k in range(1, n):
        mate, child = 2 * k, 2 * k + 1
        fa[child - 1], mo[child - 1] = (prev, mate) if k % 2 else (mate, prev)
        prev = child
    pro = np.array([3, 5, 21, 2 * n - 1, 2, 1], dtype=np.int64)
    st = _check(gen, (ind, fa, mo), pro, 1000, 8)
    assert st["levels"] == n and st["planes"] == 10


def test_half_founders_selfing_and_repeated_probands(gen):
    from test_ident_host import shapes_pedigree
    ind, fa, mo = shapes_pedigree()
    pro = np.array([8, 6, 8, 7, 5, 1, 9, 6], dtype=np.int64)
    want = IdentVector(ind, fa, mo, pro).labels(2000, 4)
    _check(gen, (ind, fa, mo), pro, 2000, 4, want=want)
    c = counts_of(want)
    assert np.array_equal(c[0, 2], c[0, 0]) and np.all(c[0, 2, [1, 2, 3, 4, 5, 7, 8]] == 0)    # repeats of one ID: states 1 and 7
    assert abs(c[1, 1, 0] / 2000 - 0.5) < 0.06                                                # 6 = (3, 3): inbreeding 1/2; both sides drew
    others = [0, 1, 2, 3, 4, 5, 7]                                                            # 9 is unrelated to them: states 4 and 9 only
    assert c[0, 0, 0] > 0 and np.all(c[others, 6][:, [0, 1, 2, 4, 5, 6, 7]] == 0) and np.all(c[5, 5] == [0, 0, 0, 0, 0, 0, 2000, 0, 0])


def test_sub_list_branching_and_other_seeds(gen, big):
    (ind, fa, mo), pro, want = big
    ped = _ped(gen, ind, fa, mo)
    full = gen.simuIdentity(ped, pro, simulNo=5000, seed=9, labels=True)
    assert full.counts.dtype == np.int32 and full.counts.shape == (40, 40, 9) and (full.simulNo, full.seed) == (5000, 9)
    _same(full.counts, counts_of(want))
    _same(full.labels, want)
    _same(full.alleles, IdentVector(ind, fa, mo, pro).alleles)
    sub = np.array([33, 3, 3, 17, 7, 39])
    part = gen.simuIdentity(ped, pro[sub], simulNo=5000, seed=9)
    _same(part.counts, np.ascontiguousarray(full.counts[np.ix_(sub, sub)]))
    assert part.labels is None and len(part.alleles) < len(full.alleles)
    pruned = gen.branching(ped, pro=pro)
    assert len(pruned) < len(ped)
    again = gen.simuIdentity(pruned, pro, simulNo=5000, seed=9, labels=True)
    _same(again.counts, full.counts)
    _same(again.labels, full.labels)
    short = gen.simuIdentity(ped, pro, simulNo=64, seed=9, labels=True)
    _same(short.labels, np.ascontiguousarray(full.labels[:, :, :64]))
    assert not np.array_equal(gen.simuIdentity(ped, pro, simulNo=5000, seed=10).counts, full.counts)
    a, b = gen.simuIdentity(ped, pro, simulNo=256), gen.simuIdentity(ped, pro, simulNo=256)
    assert a.seed != b.seed and not np.array_equal(a.counts, b.counts)                   # fresh seeds
    dflt = gen.simuIdentity(ped, simulNo=130, seed=1)                                    # pro(ped)
    _same(dflt.pro, gen.pro(ped))
    _same(dflt.counts, IdentVector(ind, fa, mo, gen.pro(ped)).counts(130, 1))


@pytest.mark.parametrize("state", [2, 1])
def test_cross_check_with_simuSample_on_genea140(gen, state):
    """GPU against GPU: 20 founders among the ancestors of genea140's first 32 probands listed as gen.simuSample's ancestors with
    state 2 (1), the same seed: a proband's count in a simulation is the number of its two labels that belong to those founders
    (to their side-0 alleles)."""
    ped = gen.genealogy(gen.genea140)
    pro, S = gen.pro(ped)[:32], 5000
    r = gen.simuIdentity(ped, pro, simulNo=S, seed=13, labels=True)
    ids, n_sides = np.unique(r.alleles[:, 0], return_counts=True)
    founders = ids[n_sides == 2]                                      # both parents unknown
    marked = founders[:: max(1, len(founders) // 20)][:20]
    assert len(marked) == 20
    sample = gen.simuSample(ped, pro, marked, np.full(20, state), simulNo=S, seed=13)
    mine = np.isin(r.alleles[:, 0], marked) & ((r.alleles[:, 1] == 0) | (state == 2))
    want = mine[r.labels].sum(axis=1).astype(np.int8)
    _same(sample, want)
    assert want.any()
    assert np.all(r.counts.sum(axis=-1) == S) and np.array_equal(swap_roles(r.counts), r.counts)


def test_simuIdentity_meets_the_exact_kinship_on_geneaJi(gen):
    """One condition, not a measurement: |kinship estimate - exact kinship| <= 5 / sqrt(S) for every pair (a per-simulation score in
    [0, 1] has a standard deviation of at most 1/2; tests/test_ident_host.py holds the reference to the same margin)."""
    ped = gen.genealogy(gen.geneaJi)
    S = 5000
    r = gen.simuIdentity(ped, simulNo=S, seed=7)
    exact = ExactKinship(*_args(ped)).float64(r.pro)
    dev = np.abs(r.kinship - exact).max() * np.sqrt(S)
    print("geneaJi, S = %d, seed 7: largest |kinship estimate - exact kinship| = %.3f / sqrt(S)" % (S, dev))
    assert dev <= 5.0
    assert r.delta.shape == (3, 3, 9) and np.array_equal(r.inbreeding, r.delta[[0, 1, 2], [0, 1, 2], 0])
    assert np.array_equal(r.fraternity, r.delta[..., 6]) and np.array_equal(r.ibd.sum(axis=-1) + r.inbred, np.ones((3, 3)))
    assert np.array_equal(r.kinship, r.kinship.T)
    f_exact = 2.0 * np.diag(exact) - 1.0
    assert np.abs(r.inbreeding - f_exact).max() * np.sqrt(S) <= 5.0


def test_labels_to_host_without_the_flag(gen):
    ped = gen.genealogy(gen.geneaJi)
    h = gen.IdentityPlan(*_args(ped), gen.pro(ped), simul_no=64, seed=1)
    try:
        h.compute()
        with pytest.raises(ValueError, match="GENPHI_IDENT_FLAG_LABELS"):
            h.labels_to_host()
        rc = gen._capi.lib().genphi_ident_labels_to_host(h._h, None)
        assert rc == gen._capi.GENPHI_ERR_ARG
        assert h.counts_to_host().sum() == 9 * 64
    finally:
        h.close()
