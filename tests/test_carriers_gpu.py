"""gen.simuCarriers on the MI355X (gen.CarriersPlan, gen.simuCarriers) against the reference of tests/carriers_oracle.py: every
comparison is np.array_equal, every handle is computed twice with equal bytes.  Shapes are the smallest at which each part of
csrc/carry.hip can go wrong: word and pair edges of the simulations, forced and ragged panels, forced and ragged label chunks, allele
tables at the plane and dword edges, numbers of cases around the number of waves of the count kernel and its unrolling, a hub couple
whose 300 children all add into the same four counters, one selfed founder with 32,767 children (both counter fields near their
ends), controls, lumped columns, and the invariants of the definition against gen.simuRetention.  A reference is computed once per
pedigree at the largest S and cut to the columns a case needs."""
import os

import numpy as np
import pytest

from carriers_oracle import CarryVector, check_invariants, counts, fill
from random_pedigree import random_pedigree
from test_ident_host import shapes_pedigree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = [1, 63, 64, 65, 127, 128, 129, 200, 5000]
WAVES = 16                                   # the count kernel's workgroup: 1,024 threads
UNROLL = 4                                   # the individuals a wave has in flight
NONE = np.zeros(0, dtype=np.int64)
DEFAULT_CHUNK = 608                          # csrc/carry.h: CARRY_DEFAULT_CHUNK, also the widest


def _args(ped):
    return ped.ind, ped.father, ped.mother


def _ped(gen, ind, fa, mo):
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b), (np.argwhere(a != b)[:5], a[a != b][:5], b[a != b][:5])


def _rule(n_labels, arg):
    """(chunk_labels, chunks, lds_bytes) as csrc/carry.h gives them."""
    lc = min(n_labels, 608, (arg + 31) // 32 * 32 if arg else DEFAULT_CHUNK)
    return lc, -(-n_labels // lc), 256 * (lc | 1)


def _by_allele(alleles, values):
    return {(int(a), int(s)): v for (a, s), v in zip(alleles.tolist(), values.tolist())}


def _check(gen, args, cases, controls, S, seed, ref=None, max_count=0, **kw):
    """The three tables of one handle, computed twice, against the reference; the invariants on the device's tables; returns stats()."""
    if ref is None:
        ref = CarryVector(*args, cases, controls, S, seed)
    want = ref.at(S, max_count)
    h = gen.CarriersPlan(*args, cases, controls, simul_no=S, seed=seed, max_count=max_count, **kw)
    try:
        _same(h.alleles(), ref.alleles)
        assert (h.n_cases, h.n_controls, h.columns) == (ref.n, len(ref.control_labels), want[0].shape[1])
        for _ in range(2):
            h.compute()
            got = h.carriers_to_host(), h.homozygotes_to_host(), h.excluded_to_host()
            for g, w in zip(got, want):
                _same(g, w)
        check_invariants(*got, h.alleles(), S, cases, controls)
        st = h.stats()
        assert st["sweep_ms"] >= 0.0 and st["count_ms"] > 0.0 and st["planes"] == h.planes
        assert (st["chunk_labels"], st["chunks"], st["lds_bytes"]) == _rule(h.n_labels, kw.get("chunk_labels", 0))
        cols = kw.get("panel_cols", 0)
        pairs = min(-(-S // 128), -(-cols // 128)) if cols else -(-S // 128)
        assert (st["panel_cols"], st["panels"]) == (128 * pairs, -(-(-(-S // 128)) // pairs))
        assert st["count_bytes"] == 2 * (h.n_cases + h.n_controls) * h.planes * 16 * -(-S // 128) * st["chunks"]
        assert st["algorithmic_bytes"] == 48 * h.planes * (2 * h.n_live - h.n_labels) * -(-S // 128)
        return st
    finally:
        h.close()


@pytest.fixture(scope="module")
def ji(gen):
    ped = gen.genealogy(gen.geneaJi)
    pro = gen.pro(ped)
    return ped, pro, CarryVector(*_args(ped), pro, None, 5000, 2024)


def _big_pedigree():
    """600 individuals with founders anywhere, half-founders and selfing; 40 cases with repeats, a non-leaf and a founder (the recipe
    of tests/test_retain_gpu.py); 10 controls: leaves, a non-leaf and a founder."""
    rng = np.random.default_rng(177)
    ind, fa, mo, _ = random_pedigree(rng, 600, p_founder=0.08, p_one_parent=0.1, p_selfing=0.03, max_back=60, max_depth=14)
    pro = rng.choice(ind[200:], size=40, replace=False).astype(np.int64)
    parents = np.union1d(fa, mo)
    founders = ind[(fa == 0) & (mo == 0)]
    inner = parents[(parents > 0) & ~np.isin(parents, founders)]
    pro[33], pro[17], pro[5], pro[8] = pro[0], pro[0], ind[0], inner[-1]
    leaves = np.setdiff1d(np.setdiff1d(ind[150:], parents), pro)
    controls = np.concatenate([leaves[::7][:8], np.setdiff1d(inner, pro)[-3:-2], np.setdiff1d(founders, pro)[1:2]]).astype(np.int64)
    return (ind, fa, mo), pro, controls


@pytest.fixture(scope="module")
def big():
    """The reference labels of the 600-individual case at S = 5000, without controls."""
    args, pro, _ = _big_pedigree()
    return args, pro, CarryVector(*args, pro, None, 5000, 9)


@pytest.fixture(scope="module")
def big_controls():
    args, pro, controls = _big_pedigree()
    return args, pro, controls, CarryVector(*args, pro, controls, 5000, 9)


@pytest.mark.parametrize("S", EDGES)
def test_word_and_pair_edges(gen, ji, S):
    ped, pro, ref = ji
    st = _check(gen, _args(ped), pro, None, S, 2024, ref=ref)
    assert st["panels"] == 1 and st["chunks"] == 1


def test_big_case_has_the_shapes_it_claims(big, big_controls):
    (ind, fa, mo), pro, ref = big
    o = ref.o
    assert o.levels >= 5 and o.n_live >= 150 and o.planes >= 6 and o.n_labels > 64
    assert ref.n == 38 and fa[ind == pro[5]][0] == 0 and mo[ind == pro[5]][0] == 0 and np.isin(pro[8], np.union1d(fa, mo))
    carriers, homozygotes, excluded = ref.at(5000)
    assert np.any(carriers[:, 4:]) and np.any(homozygotes[:, 1:]) and not excluded.any()
    _, _, controls, rc = big_controls
    parents = np.union1d(fa, mo)
    assert len(np.unique(controls)) == 10 and not np.any(np.isin(controls, pro))
    assert np.any(~np.isin(controls, parents)) and np.any(np.isin(controls, parents) & ((fa[controls - 1] > 0) | (mo[controls - 1] > 0))) and np.any((fa[controls - 1] == 0) & (mo[controls - 1] == 0))
    assert rc.n_labels >= o.n_labels and np.any((rc.at(5000)[2] > 0) & (rc.at(5000)[2] < 5000))


def test_forced_panels(gen, big):
    args, pro, ref = big
    for cols, panels in ((128, 40), (1000, 5), (5000, 1), (0, 1)):
        st = _check(gen, args, pro, None, 5000, 9, ref=ref, panel_cols=cols)
        assert st["panels"] == panels


def test_forced_chunks(gen, big):
    """Chunks of 32 and 64 labels and the default; the last chunk is ragged, asserted from the allele table first.  Then ragged panels
    and ragged chunks at once."""
    args, pro, ref = big
    n = ref.n_labels
    for lc in (32, 64):
        assert n % lc != 0, "the last chunk is not ragged"
        st = _check(gen, args, pro, None, 5000, 9, ref=ref, chunk_labels=lc)
        assert st["chunks"] == -(-n // lc) >= 2
    st = _check(gen, args, pro, None, 5000, 9, ref=ref)
    assert st["chunks"] == 1 and n < DEFAULT_CHUNK
    st = _check(gen, args, pro, None, 1000, 9, ref=ref, chunk_labels=32, panel_cols=384)
    assert st["panels"] == 3 and 8 % 3 != 0 and st["chunks"] >= 2


def _founders_and_sibships(n_full, n_half):
    """n_full unrelated founders and n_half half-founders (children of founder 1 with an unknown mother); three children of
    founders 1 and 2 (of founder 1 selfed when it is alone); a child of the last two.  2 n_full + n_half labels.  (The shapes of
    tests/test_retain_gpu.py, rebuilt here.)"""
    ind = list(range(1, n_full + 1))
    fa, mo = [0] * n_full, [0] * n_full
    mate = 2 if n_full >= 2 else 1
    for _ in range(3):
        ind.append(len(ind) + 1)
        fa.append(1)
        mo.append(mate)
    for _ in range(n_half):
        ind.append(len(ind) + 1)
        fa.append(1)
        mo.append(0)
    ind.append(len(ind) + 1)
    fa.append(ind[-2])
    mo.append(ind[-3])
    return np.array(ind, dtype=np.int64), np.array(fa, dtype=np.int64), np.array(mo, dtype=np.int64)


@pytest.mark.parametrize("n_full,n_half", [(1, 0), (1, 1), (15, 1), (16, 0), (15, 3), (31, 1), (32, 0), (31, 3), (128, 1)])
def test_allele_tables_at_the_plane_and_dword_edges(gen, n_full, n_half):
    """2, 3, 31, 32, 33, 63, 64, 65 and 257 labels: the plane edges of the sweep, a table that ends on a chunk of 32 or of 256 and
    one label past it.  Everyone is a case."""
    ind, fa, mo = _founders_and_sibships(n_full, n_half)
    n_labels = 2 * n_full + n_half
    ref = CarryVector(ind, fa, mo, ind, None, 200, 3)
    assert (ref.n_labels, ref.o.planes) == (n_labels, max(1, (n_labels - 1).bit_length()))
    st = _check(gen, (ind, fa, mo), ind, None, 200, 3, ref=ref)
    assert st["chunks"] == 1
    if n_labels > 32:
        _check(gen, (ind, fa, mo), ind, None, 200, 3, ref=ref, chunk_labels=32)
    if n_labels > 256:
        assert _check(gen, (ind, fa, mo), ind, None, 200, 3, ref=ref, chunk_labels=256)["chunks"] == 2


@pytest.fixture(scope="module")
def clan():
    """200 individuals in few generations, closely related: the pool the case-count tests draw from."""
    rng = np.random.default_rng(3)
    ind, fa, mo, _ = random_pedigree(rng, 200, p_founder=0.1, p_one_parent=0.05, p_selfing=0.05, max_back=20)
    return (ind, fa, mo), rng.permutation(ind)


@pytest.mark.parametrize("n", [1, 2, 3, WAVES - 1, WAVES, WAVES + 1, WAVES * UNROLL - 1, WAVES * UNROLL, WAVES * UNROLL + 1, 129])
def test_numbers_of_cases(gen, clan, n):
    """1, 2, 3; the number of waves +- 1; the waves times the unrolling +- 1; 129.  Three controls move the border between the two
    parts of the row list across the same edges."""
    args, order = clan
    _check(gen, args, order[:n], None, 200, 5)
    _check(gen, args, order[:n], order[150:153], 200, 5)


def test_hub_couple_with_300_children(gen):
    """Every wave adds into the same four counters: c1 + c1' = 300 per parent and simulation.  A single count is Binomial(300, 1/2)
    there (mean 150, standard deviation 8.7) and cannot pass 255, so a second shape follows: 300 more cases, the children of one of
    the 300 selfed, carry two of the couple's alleles with probability 3/4 each, and the counts pass 255 with both fields in use."""
    ind = np.arange(1, 303, dtype=np.int64)
    fa = np.where(ind > 2, 1, 0).astype(np.int64)
    mo = np.where(ind > 2, 2, 0).astype(np.int64)
    cases = ind[2:]
    ref = CarryVector(ind, fa, mo, cases, None, 200, 3)
    c1, c2 = counts(ref.case_labels, 4)
    assert np.all(c1[0] + c1[1] == 300) and np.all(c1[2] + c1[3] == 300) and not c2.any()
    st = _check(gen, (ind, fa, mo), cases, None, 200, 3, ref=ref)
    assert st["levels"] == 2 and st["planes"] == 2 and st["columns"] == 301
    ind2 = np.arange(1, 603, dtype=np.int64)
    fa2 = np.concatenate([fa, np.full(300, 3)]).astype(np.int64)
    mo2 = np.concatenate([mo, np.full(300, 3)]).astype(np.int64)                  # 3 selfed: its children carry two of the couple's alleles
    cases2 = ind2[2:]
    ref2 = CarryVector(ind2, fa2, mo2, cases2, None, 200, 3)
    c1, c2 = counts(ref2.case_labels, 4)
    assert c1.max() > 255 and c2.max() > 64 and np.all(c1[0] + c1[1] >= 300) and np.all((c1 + c2).sum(axis=0) == 1200)
    _check(gen, (ind2, fa2, mo2), cases2, None, 200, 3, ref=ref2)


def test_both_counter_fields_near_their_ends(gen):
    """One founder selfed, 32,767 children as cases, S = 64: c1 of either allele is about 3/4 of them, c2 about 1/4.  Also with
    max_count = 3, the lumped column.  (The reference is IdentVector's: it takes under a second at this size.)"""
    n = 32767
    ind = np.arange(1, n + 2, dtype=np.int64)
    fa = np.where(ind > 1, 1, 0).astype(np.int64)
    mo = fa.copy()
    cases = ind[1:]
    ref = CarryVector(ind, fa, mo, cases, None, 64, 11)
    c1, c2 = counts(ref.case_labels, 2)
    assert c1.min() > 16384 and c2.min() > 4096 and np.all(c1[0] + c1[1] + c2[0] + c2[1] == 2 * n)
    st = _check(gen, (ind, fa, mo), cases, None, 64, 11, ref=ref)
    assert (st["columns"], st["n_cases"], st["planes"]) == (n + 1, n, 1)
    st = _check(gen, (ind, fa, mo), cases, None, 64, 11, ref=ref, max_count=3)
    assert st["columns"] == 4
    carriers, homozygotes, _ = ref.at(64, 3)
    assert carriers[:, 3].tolist() == [64, 64] and homozygotes[:, 3].tolist() == [64, 64]


def test_half_founders_selfing_and_repeated_cases(gen):
    ind, fa, mo = shapes_pedigree()
    cases = np.array([8, 6, 8, 5, 1, 6], dtype=np.int64)
    ref = CarryVector(ind, fa, mo, cases, [9, 7, 9], 2000, 4)
    _check(gen, (ind, fa, mo), cases, [9, 7, 9], 2000, 4, ref=ref)
    _check(gen, (ind, fa, mo), np.array([6], dtype=np.int64), None, 2000, 4)                 # 6 = (3, 3): one selfed case alone
    carriers, homozygotes, excluded = ref.at(2000)
    key = {(int(a), int(s)): k for k, (a, s) in enumerate(ref.alleles.tolist())}
    assert excluded[key[(9, 0)]] == excluded[key[(9, 1)]] == excluded[key[(7, 0)]] == 2000       # the controls' own founder sides
    assert carriers[key[(1, 0)], 1:].sum() + excluded[key[(1, 0)]] == 2000 and np.any(homozygotes[key[(1, 0)], 1:])    # 1 is a case; 6 is selfed


def test_controls(gen, big, big_controls):
    """10 controls: leaves, a non-leaf and a founder.  The founder's own alleles have excluded == S.  Invariant 6: excluded equals
    gen.simuRetention's survived on the controls alone; invariant 7: adding controls never raises a cell with c >= 1."""
    args, pro, controls, ref = big_controls
    S = 5000
    _check(gen, args, pro, controls, S, 9, ref=ref)
    _check(gen, args, pro, controls, 1000, 9, ref=ref, chunk_labels=32, panel_cols=384, max_count=2)
    ped = _ped(gen, *args)
    r = gen.simuCarriers(ped, pro, controls, simulNo=S, seed=9)
    ind, fa, mo = args
    founder = controls[(fa[controls - 1] == 0) & (mo[controls - 1] == 0)]
    assert len(founder) == 1 and np.all(r.excluded[r.alleles[:, 0] == founder[0]] == S) and np.sum(r.alleles[:, 0] == founder[0]) == 2
    kept = gen.simuRetention(ped, controls, simulNo=S, seed=9, contributions=False)                 # 6
    mine, theirs = _by_allele(r.alleles, r.excluded), _by_allele(kept.alleles, kept.survived)
    common = set(mine) & set(theirs)
    assert any(0 < mine[k] < S for k in common) and set(theirs) <= set(mine)
    assert all(mine[k] == theirs[k] for k in common) and all(mine[k] == 0 for k in set(mine) - common)
    plain = gen.simuCarriers(ped, pro, simulNo=S, seed=9)                                            # 7
    for with_c, without in ((r.carriers, plain.carriers), (r.homozygotes, plain.homozygotes)):
        a, b = _by_allele(r.alleles, with_c[:, 1:]), _by_allele(plain.alleles, without[:, 1:])
        assert set(b) <= set(a) and all(np.all(np.asarray(a[k]) <= np.asarray(b[k])) for k in b)
        assert any(np.any(np.asarray(a[k]) < np.asarray(b[k])) for k in b) and all(not np.any(a[k]) for k in set(a) - set(b))
    _same(plain.carriers, fill(big[2].at(S)[0], plain.excluded, S))


def test_the_carriers_are_the_survivors_of_retention(gen, big):
    """Invariant 1, both handles on the device: with no controls the sum over c >= 1 of carriers is gen.RetentionPlan's survived."""
    args, pro, _ = big
    for S, cols, lc in ((5000, 0, 0), (333, 128, 32)):
        g = gen.RetentionPlan(*args, pro, simul_no=S, seed=77, panel_cols=cols, chunk_labels=lc)
        h = gen.CarriersPlan(*args, pro, simul_no=S, seed=77, panel_cols=cols, chunk_labels=lc)
        try:
            g.compute()
            h.compute()
            _same(h.alleles(), g.alleles())
            assert h.stats()["sweep_ms"] > 0.0
            _same(h.carriers_to_host()[:, 1:].sum(axis=1, dtype=np.int64).astype(np.int32), g.survived_to_host())
            assert not h.excluded_to_host().any()
        finally:
            g.close()
            h.close()


@pytest.mark.parametrize("max_count", [1, 2, 37])
def test_max_count(gen, big, big_controls, max_count):
    """1, 2 and n - 1 (38 distinct cases) against the reference's clamped tables; the clamped tables are the full ones with the tail
    summed into the last column."""
    args, pro, ref = big
    assert ref.n - 1 == 37
    st = _check(gen, args, pro, None, 5000, 9, ref=ref, max_count=max_count)
    assert st["columns"] == max_count + 1
    full, cut = ref.at(5000), ref.at(5000, max_count)
    for f, c in zip(full[:2], cut[:2]):
        assert np.array_equal(c[:, :max_count], f[:, :max_count]) and np.array_equal(c[:, max_count], f[:, max_count:].sum(axis=1))
    _, _, controls, rc = big_controls
    _check(gen, args, pro, controls, 5000, 9, ref=rc, max_count=max_count)
    ped = _ped(gen, *args)
    r = gen.simuCarriers(ped, pro, simulNo=5000, seed=9, maxCount=max_count)
    assert r.lumped and r.prob_all is None and r.posterior is None
    _same(r.carriers, fill(cut[0], cut[2], 5000))
    _same(r.at_least(max_count), full[0][:, max_count:].sum(axis=1, dtype=np.int64) / 5000.0)


def test_order_repeats_branching_and_seeds(gen, big_controls):
    (ind, fa, mo), pro, controls, ref = big_controls
    ped = _ped(gen, ind, fa, mo)
    S = 5000
    want = ref.at(S)

    def run(p, c, seed=9, S=S, pedigree=ped):
        r = gen.simuCarriers(pedigree, p, c, simulNo=S, seed=seed)
        return r, (r.carriers, r.homozygotes, r.excluded)

    full, got = run(pro, controls)
    _same(full.alleles, ref.alleles)
    _same(full.pro, np.unique(pro))
    _same(full.controls, np.unique(controls))
    assert (full.simulNo, full.seed, full.lumped) == (S, 9, False)
    for g, w in zip(got[:2], want[:2]):
        _same(g, fill(w, want[2], S))
    _same(got[2], want[2])
    rng = np.random.default_rng(4)
    for p, c in ((np.unique(pro), np.unique(controls)), (rng.permutation(pro), rng.permutation(controls)),
                 (np.concatenate([pro, pro[:7]]), np.concatenate([controls[::-1], controls[:3]]))):
        r, again = run(p, c)
        _same(r.alleles, full.alleles)
        for g, w in zip(again, got):
            assert g.tobytes() == w.tobytes()
    pruned = gen.branching(ped, pro=np.concatenate([pro, controls]))
    assert len(pruned) < len(ped)
    r, again = run(pro, controls, pedigree=pruned)
    _same(r.alleles, full.alleles)
    for g, w in zip(again, got):
        _same(g, w)
    assert not np.array_equal(run(pro, controls, seed=10)[1][0], full.carriers)
    a, b = gen.simuCarriers(ped, pro, controls, simulNo=256), gen.simuCarriers(ped, pro, controls, simulNo=256)
    assert a.seed != b.seed and not np.array_equal(a.carriers, b.carriers)                        # fresh seeds
    replay = gen.simuCarriers(ped, pro, controls, simulNo=256, seed=a.seed)
    for g, w in zip((replay.carriers, replay.homozygotes, replay.excluded), (a.carriers, a.homozygotes, a.excluded)):
        _same(g, w)


def test_two_founders_with_three_children_as_cases(gen):
    """A derivable bound at S = 5000.  Each of the three children carries a given allele of a parent with probability 1/2,
    independently: the number of carriers is Binomial(3, 1/2), the shares of c = 0, 1, 2, 3 are 1/8, 3/8, 3/8, 1/8.  A Bernoulli
    share's standard deviation is at most 0.5 / sqrt(S): the margin 5 / sqrt(S) is ten standard deviations.  No child is homozygous."""
    ind = np.arange(1, 6, dtype=np.int64)
    fa = np.array([0, 0, 1, 1, 1], dtype=np.int64)
    mo = np.array([0, 0, 2, 2, 2], dtype=np.int64)
    S = 5000
    r = gen.simuCarriers(_ped(gen, ind, fa, mo), ind[2:], simulNo=S, seed=12)
    assert r.alleles.tolist() == [[1, 0], [1, 1], [2, 0], [2, 1]] and r.founders.tolist() == [1, 2] and r.carriers.shape == (4, 4)
    assert np.all(r.carriers.sum(axis=1) == S) and not r.excluded.any()
    dev = np.abs(r.carriers / float(S) - np.array([1, 3, 3, 1]) / 8.0).max() * np.sqrt(S)
    print("two founders, three children, S = %d: the largest deviation of a share is %.3f / sqrt(S)" % (S, dev))
    assert dev <= 5.0
    assert not r.homozygotes[:, 1:].any() and np.all(r.homozygotes[:, 0] == S)
    assert abs(r.posterior.sum() - 1.0) <= 1e-12 and np.array_equal(r.prob_all, r.carriers[:, 3] / float(S))
    assert np.array_equal(r.at_least(1), r.carriers[:, 1:].sum(axis=1) / float(S)) and np.array_equal(r.at_least(0), np.ones(4))
    assert sorted(r.ranking.tolist()) == [0, 1, 2, 3] and np.all(np.diff(r.prob_all[r.ranking]) <= 0)


@pytest.mark.parametrize("name", ["geneaJi", "genea140"])
def test_simuCarriers_end_to_end(gen, name):
    ped = gen.genealogy(getattr(gen, name))
    if name == "geneaJi":
        S, cases, controls = 5000, gen.pro(ped), NONE
        r = gen.simuCarriers(ped, simulNo=S, seed=21)
    else:
        S = 1000
        pop = gen._pop(os.path.join(ROOT, "tests", "golden", "pop140.csv"))
        cases = np.array(sorted(k for k, v in pop.items() if v == "Saguenay"), dtype=np.int64)
        controls = np.array(sorted(k for k, v in pop.items() if v == "Quebec"), dtype=np.int64)
        assert len(cases) == 22 and len(controls) == 16
        r = gen.simuCarriers(ped, cases, controls, simulNo=S, seed=21)
    _same(r.pro, np.unique(cases))
    _same(r.controls, np.unique(controls))
    h = gen.CarriersPlan(*_args(ped), cases, controls, simul_no=S, seed=21)
    try:
        for _ in range(2):
            h.compute()
            got = h.carriers_to_host(), h.homozygotes_to_host(), h.excluded_to_host()
            _same(r.carriers[:, 1:], got[0][:, 1:])
            _same(r.homozygotes[:, 1:], got[1][:, 1:])
            _same(r.excluded, got[2])
            assert not got[0][:, 0].any() and not got[1][:, 0].any()
        _same(r.alleles, h.alleles())
        assert h.stats()["chunks"] == -(-h.n_labels // DEFAULT_CHUNK)
    finally:
        h.close()
    check_invariants(r.carriers, r.homozygotes, r.excluded, r.alleles, S, cases, controls)
    check_invariants(*got, r.alleles, S, cases, controls)
    assert np.all(r.carriers.sum(axis=1, dtype=np.int64) + r.excluded == S) and np.all(r.homozygotes.sum(axis=1, dtype=np.int64) + r.excluded == S)
    assert r.carriers.shape == (len(r.alleles), len(cases) + 1) and not r.lumped
    assert np.all((r.at_least(1) >= 0.0) & (r.at_least(1) <= 1.0)) and np.all(r.mean_carriers >= r.at_least(1))
    if name == "genea140":
        assert np.any((r.excluded > 0) & (r.excluded < S)) and np.any(r.carriers[:, 2:])
    fresh = gen.simuCarriers(ped, cases, controls, simulNo=256)
    replay = gen.simuCarriers(ped, cases, controls, simulNo=256, seed=fresh.seed)
    _same(replay.carriers, fresh.carriers)
    _same(replay.homozygotes, fresh.homozygotes)
    _same(replay.excluded, fresh.excluded)
