"""gen.simuRetention on the MI355X (gen.RetentionPlan, gen.simuRetention) against the reference of tests/retain_oracle.py: every
comparison is np.array_equal, every handle is computed twice with equal bytes.  Shapes are the smallest at which each part of
csrc/retain.hip can go wrong: word and pair edges of the simulations, forced and ragged panels, forced and ragged label chunks with
a founder split by a chunk border, allele tables at the plane and dword edges of a bitmap, proband counts around the number of
waves of the mark kernel and its unrolling, a hub couple whose children all mark the same bits (both forms of the mark phase), a
deep chain, half-founders, selfing and repeats.  A reference is computed once per pedigree at the largest S and cut to the columns
a case needs (the prefix rule of the definition, checked on the reference itself in tests/test_retain_host.py)."""
import numpy as np
import pytest

from ident_oracle import IdentVector
from random_pedigree import random_pedigree
from retain_oracle import RetainVector, check_invariants, reductions

pytestmark = pytest.mark.gpu

EDGES = [1, 63, 64, 65, 127, 128, 129, 200, 5000]
WAVES = 16                                   # the mark kernel's workgroup: 1,024 threads


def _args(ped):
    return ped.ind, ped.father, ped.mother


def _ped(gen, ind, fa, mo):
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b), (np.argwhere(a != b)[:5], a[a != b][:5], b[a != b][:5])


def _rule(n_labels, arg):
    """(chunk_labels, chunks, lds_bytes) as csrc/retain.h gives them."""
    lc = min(n_labels, 16384, (arg + 31) // 32 * 32 if arg else 8192)
    return lc, -(-n_labels // lc), 256 * ((lc // 32 + 1) | 1)


def _check(gen, args, pro, S, seed, ref=None, **kw):
    """The three arrays of one handle, computed twice, against the reference; the invariants on the device's arrays; returns stats()."""
    if ref is None:
        ref = RetainVector(*args, pro, S, seed)
    want = ref.at(S)
    h = gen.RetentionPlan(*args, pro, simul_no=S, seed=seed, **kw)
    try:
        _same(h.alleles(), ref.alleles)
        for _ in range(2):
            h.compute()
            got = h.survived_to_host(), h.both_to_host(), h.distinct_to_host()
            for g, w in zip(got, want):
                _same(g, w)
        check_invariants(*got, h.alleles(), S, pro)
        st = h.stats()
        assert st["sweep_ms"] >= 0.0 and st["mark_ms"] > 0.0 and st["planes"] == h.planes
        assert (st["chunk_labels"], st["chunks"], st["lds_bytes"]) == _rule(h.n_labels, kw.get("chunk_labels", 0))
        cols = kw.get("panel_cols", 0)
        pairs = min(-(-S // 128), -(-cols // 128)) if cols else -(-S // 128)
        assert (st["panel_cols"], st["panels"]) == (128 * pairs, -(-(-(-S // 128)) // pairs))
        assert st["mark_bytes"] == 2 * len(pro) * h.planes * 16 * -(-S // 128) * st["chunks"]
        assert st["algorithmic_bytes"] == 48 * h.planes * (2 * h.n_live - h.n_labels) * -(-S // 128)
        return st
    finally:
        h.close()


@pytest.fixture(scope="module")
def ji(gen):
    ped = gen.genealogy(gen.geneaJi)
    pro = gen.pro(ped)
    return ped, pro, RetainVector(*_args(ped), pro, 5000, 2024)


@pytest.fixture(scope="module")
def big():
    """600 individuals with founders anywhere, half-founders and selfing; 40 probands with repeats, a non-leaf and a founder; the
    reference labels at S = 5000."""
    rng = np.random.default_rng(177)
    ind, fa, mo, _ = random_pedigree(rng, 600, p_founder=0.08, p_one_parent=0.1, p_selfing=0.03, max_back=60, max_depth=14)
    pro = rng.choice(ind[200:], size=40, replace=False).astype(np.int64)
    parents = np.union1d(fa, mo)
    non_leaf = parents[(parents > 0) & ~np.isin(parents, ind[(fa == 0) & (mo == 0)])][-1]
    pro[33], pro[17], pro[5], pro[8] = pro[0], pro[0], ind[0], non_leaf
    return (ind, fa, mo), pro, RetainVector(ind, fa, mo, pro, 5000, 9)


@pytest.mark.parametrize("S", EDGES)
def test_word_and_pair_edges(gen, ji, S):
    ped, pro, ref = ji
    st = _check(gen, _args(ped), pro, S, 2024, ref=ref)
    assert st["panels"] == 1 and st["chunks"] == 1


def test_big_case_has_the_shapes_it_claims(big):
    (ind, fa, mo), pro, ref = big
    o = ref.o
    assert o.levels >= 5 and o.n_live >= 150 and o.planes >= 6 and o.n_labels > 64
    lf, lm = o.fa[o.live], o.mo[o.live]
    assert np.any((lf >= 0) & (lf == lm)) and np.any((lf < 0) != (lm < 0))               # selfing, half-founders
    assert len(np.unique(pro)) == 38 and fa[ind == pro[5]][0] == 0 and mo[ind == pro[5]][0] == 0 and np.isin(pro[8], np.union1d(fa, mo))
    survived, both, distinct = ref.at(5000)
    assert np.any(survived == 5000) and np.any((survived > 0) & (survived < 5000)) and np.any((both > 0) & (both < survived))
    assert len(np.unique(distinct)) > 5


def test_forced_panels(gen, big):
    args, pro, ref = big
    for cols, panels in ((128, 40), (1000, 5), (5000, 1), (100000, 1), (0, 1)):
        st = _check(gen, args, pro, 5000, 9, ref=ref, panel_cols=cols)
        assert st["panels"] == panels


@pytest.mark.parametrize("mark", [None, "or", "test"])
def test_forced_chunks(gen, big, mark):
    """Chunks of 32 and 64 labels and the default: a border splits a founder's two labels (its `both` needs the halo bit) and the
    last chunk is ragged.  Both are asserted from the allele table first."""
    args, pro, ref = big
    ids, n = ref.alleles[:, 0], len(ref.alleles)
    for lc in (32, 64):
        borders = np.arange(lc, n, lc)
        assert len(borders) >= 1 and np.any(ids[borders - 1] == ids[borders]), "no founder is split by a chunk border"
        assert n % lc != 0, "the last chunk is not ragged"
        st = _check(gen, args, pro, 5000, 9, ref=ref, chunk_labels=lc, mark=mark)
        assert st["chunks"] == -(-n // lc) >= 2
    st = _check(gen, args, pro, 5000, 9, ref=ref, mark=mark)
    assert st["chunks"] == 1
    _check(gen, args, pro, 1000, 9, ref=ref, chunk_labels=32, panel_cols=384, mark=mark)       # ragged panels and ragged chunks at once


def _founders_and_sibships(n_full, n_half):
    """n_full unrelated founders and n_half half-founders (children of founder 1 with an unknown mother); three children of
    founders 1 and 2 (of founder 1 selfed when it is alone); everyone is a proband.  2 n_full + n_half labels."""
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
    ind.append(len(ind) + 1)                                                    # a child of the last two: an inbred or half-founder line
    fa.append(ind[-2])
    mo.append(ind[-3])
    return np.array(ind, dtype=np.int64), np.array(fa, dtype=np.int64), np.array(mo, dtype=np.int64)


@pytest.mark.parametrize("n_full,n_half", [(1, 0), (1, 1), (15, 1), (16, 0), (15, 3), (31, 1), (32, 0), (31, 3), (128, 1)])
def test_allele_tables_at_the_plane_and_dword_edges(gen, n_full, n_half):
    """2, 3, 31, 32, 33, 63, 64, 65 and 257 labels: the plane edges of the sweep and the dword edges of a bitmap (at a multiple of 32
    the halo bit opens a dword of its own)."""
    ind, fa, mo = _founders_and_sibships(n_full, n_half)
    n_labels = 2 * n_full + n_half
    h = gen.RetentionPlan(ind, fa, mo, ind, simul_no=200, seed=3)
    assert (h.n_labels, h.planes) == (n_labels, max(1, (n_labels - 1).bit_length()))
    h.close()
    ref = RetainVector(ind, fa, mo, ind, 200, 3)
    st = _check(gen, (ind, fa, mo), ind, 200, 3, ref=ref)
    assert st["lds_bytes"] == 256 * ((n_labels // 32 + 1) | 1)
    if n_labels > 32:
        _check(gen, (ind, fa, mo), ind, 200, 3, ref=ref, chunk_labels=32)


@pytest.fixture(scope="module")
def clan():
    """200 individuals in few generations, closely related: the pool the proband-count cases draw from."""
    rng = np.random.default_rng(3)
    ind, fa, mo, _ = random_pedigree(rng, 200, p_founder=0.1, p_one_parent=0.05, p_selfing=0.05, max_back=20)
    return (ind, fa, mo), rng.permutation(ind)


@pytest.mark.parametrize("n", [1, 2, 3, WAVES // 2 - 1, WAVES // 2, WAVES // 2 + 1, 2 * WAVES - 1, 2 * WAVES, 2 * WAVES + 1, 129])
def test_numbers_of_probands(gen, clan, n):
    """1, 2, 3; 2 n sides at the number of waves +- 1 and at the waves times the unrolling +- 1; 129."""
    args, order = clan
    _check(gen, args, order[:n], 200, 5)


@pytest.mark.parametrize("mark", ["or", "test"])
def test_hub_couple_with_300_children(gen, mark):
    ind = np.arange(1, 303, dtype=np.int64)
    fa = np.where(ind > 2, 1, 0).astype(np.int64)
    mo = np.where(ind > 2, 2, 0).astype(np.int64)
    pro = ind[2:]
    ref = RetainVector(ind, fa, mo, pro, 200, 3)
    st = _check(gen, (ind, fa, mo), pro, 200, 3, ref=ref, mark=mark)
    assert st["levels"] == 2 and st["planes"] == 2
    survived, both, distinct = ref.at(200)
    assert np.all(survived == 200) and both.tolist() == [200, 0, 200, 0] and np.all(distinct == 4)      # 300 children: nothing is lost


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
    _check(gen, (ind, fa, mo), pro, 1000, 8, chunk_labels=96)


def test_half_founders_selfing_and_repeated_probands(gen):
    from test_ident_host import shapes_pedigree
    ind, fa, mo = shapes_pedigree()
    pro = np.array([8, 6, 8, 7, 5, 1, 9, 6], dtype=np.int64)
    ref = RetainVector(ind, fa, mo, pro, 2000, 4)
    _check(gen, (ind, fa, mo), pro, 2000, 4, ref=ref)
    _check(gen, (ind, fa, mo), np.array([6], dtype=np.int64), 2000, 4)                       # 6 = (3, 3): one selfed proband alone
    survived, both, _ = ref.at(2000)
    assert survived.tolist()[:2] == [2000, 2000] and both[0] == 2000 and survived[-1] == survived[-2] == both[-2] == 2000    # 1 and 9 are listed


def test_order_repeats_subsets_branching_and_seeds(gen, big):
    (ind, fa, mo), pro, ref = big
    ped = _ped(gen, ind, fa, mo)
    S = 5000
    want = ref.at(S)

    def run(p, seed=9, S=S, pedigree=ped):
        r = gen.simuRetention(pedigree, p, simulNo=S, seed=seed, contributions=False)
        return r, (r.survived, r.both, r.distinct)

    full, got = run(pro)
    for g, w in zip(got, want):
        _same(g, w)
    _same(full.alleles, ref.alleles)
    assert (full.simulNo, full.seed, full.p) == (S, 9, None)
    rng = np.random.default_rng(4)
    for other in (np.unique(pro), rng.permutation(pro), np.concatenate([pro, pro[:7]])):        # 5: the set alone counts
        r, again = run(other)
        _same(r.alleles, full.alleles)
        for g, w in zip(again, got):
            assert g.tobytes() == w.tobytes()
    sub = np.unique(pro)[::3]                                                                     # 9: a sub-list and its superset
    part, _ = run(sub)
    big_map = {(int(a), int(s)): int(v) for (a, s), v in zip(full.alleles.tolist(), full.survived.tolist())}
    small = {(int(a), int(s)): int(v) for (a, s), v in zip(part.alleles.tolist(), part.survived.tolist())}
    assert set(small) <= set(big_map) and all(small[k] <= big_map[k] for k in small) and any(small[k] < big_map[k] for k in small)
    pruned = gen.branching(ped, pro=pro)                                                          # 8
    assert len(pruned) < len(ped)
    r, again = run(pro, pedigree=pruned)
    _same(r.alleles, full.alleles)
    for g, w in zip(again, got):
        _same(g, w)
    _same(run(pro, S=64)[1][2], np.ascontiguousarray(full.distinct[:64]))                          # 7
    assert not np.array_equal(run(pro, seed=10)[1][0], full.survived)
    a, b = gen.simuRetention(ped, pro, simulNo=256, contributions=False), gen.simuRetention(ped, pro, simulNo=256, contributions=False)
    assert a.seed != b.seed and not np.array_equal(a.distinct, b.distinct)                        # fresh seeds


def test_the_two_handles_agree_on_the_device(gen, big):
    """10: the three arrays are the reference's reductions of the labels that gen.IdentityPlan(labels=True) computes on the device."""
    args, pro, _ = big
    for S, cols, lc in ((5000, 0, 0), (333, 128, 32)):
        g = gen.IdentityPlan(*args, pro, simul_no=S, seed=77, labels=True, panel_cols=cols)
        h = gen.RetentionPlan(*args, pro, simul_no=S, seed=77, panel_cols=cols, chunk_labels=lc)
        try:
            g.compute()
            h.compute()
            _same(h.alleles(), g.alleles())
            want = reductions(g.labels_to_host(), g.alleles())
            for got, w in zip((h.survived_to_host(), h.both_to_host(), h.distinct_to_host()), want):
                _same(got, w)
        finally:
            g.close()
            h.close()


def test_two_founders_with_three_listed_children(gen):
    """Derivable bounds at S = 5000.  An allele of a parent misses each of k = 3 children with probability 1/2: it survives with
    probability 1 - 2^-3, a Bernoulli share whose standard deviation is below 0.5 / sqrt(S); both alleles of a parent survive unless
    all three children drew the same one: 1 - 2 x 2^-3.  The margin 5 / sqrt(S) is ten standard deviations.  A child always carries
    one of its parent's two alleles: lost = 0 exactly."""
    ind = np.arange(1, 6, dtype=np.int64)
    fa = np.array([0, 0, 1, 1, 1], dtype=np.int64)
    mo = np.array([0, 0, 2, 2, 2], dtype=np.int64)
    S = 5000
    r = gen.simuRetention(_ped(gen, ind, fa, mo), ind[2:], simulNo=S, seed=12)
    assert r.alleles.tolist() == [[1, 0], [1, 1], [2, 0], [2, 1]] and r.founders.tolist() == [1, 2] and r.n_alleles.tolist() == [2, 2]
    dev = np.abs(r.retention - (1 - 2.0**-3)).max() * np.sqrt(S)
    dev_both = np.abs(r.whole - (1 - 2 * 2.0**-3)).max() * np.sqrt(S)
    print("two founders, three children, S = %d: largest deviations %.3f / sqrt(S) (retention), %.3f / sqrt(S) (whole)" % (S, dev, dev_both))
    assert dev <= 5.0 and dev_both <= 5.0
    assert r.lost.tolist() == [0.0, 0.0]
    assert np.array_equal(r.both[[0, 2]] / float(S), r.whole) and r.distinct.min() >= 2 and r.distinct.max() <= 4


@pytest.mark.parametrize("name", ["geneaJi", "genea140"])
def test_simuRetention_end_to_end(gen, name):
    ped = gen.genealogy(getattr(gen, name))
    pro = gen.pro(ped)
    S = 5000 if name == "geneaJi" else 1000
    r = gen.simuRetention(ped, simulNo=S, seed=21)
    _same(r.pro, pro)
    h = gen.RetentionPlan(*_args(ped), pro, simul_no=S, seed=21)
    try:
        h.compute()
        _same(r.survived, h.survived_to_host())
        _same(r.both, h.both_to_host())
        _same(r.distinct, h.distinct_to_host())
        _same(r.alleles, h.alleles())
    finally:
        h.close()
    check_invariants(r.survived, r.both, r.distinct, r.alleles, S, pro)
    assert abs(r.p.sum() - 1.0) <= 1e-12 and r.p.min() > 0.0 and r.fe >= r.fg > 0.0
    assert r.alleles_mean == r.distinct.sum() / S and int(r.hist.sum()) == S and len(r.founders) == len(r.kept) == len(r.lost) == len(r.whole)
    assert np.all((r.lost >= 0.0) & (r.lost <= 1.0)) and np.all(r.kept >= r.retention.min())
    fresh = gen.simuRetention(ped, simulNo=256, contributions=False)
    replay = gen.simuRetention(ped, simulNo=256, seed=fresh.seed, contributions=False)
    _same(replay.survived, fresh.survived)
    _same(replay.both, fresh.both)
    _same(replay.distinct, fresh.distinct)
