"""gen.simuUniqueness on the MI355X (gen.UniquenessPlan, gen.simuUniqueness) against the reference of tests/uniqueness_oracle.py:
every comparison is np.array_equal, every handle is computed twice with equal bytes.  Shapes are the smallest at which each part of
csrc/unique.hip can go wrong: word and pair edges of the simulations, forced and ragged panels crossed with forced and ragged label
chunks on an allele table of a few thousand labels, allele tables at the edges of the 16-bit packing (two labels to a dword), numbers
of probands around the number of waves of the count kernel and its unrolling, numbers of others, a hub couple whose children push a
16-bit field past 255 with both halves of its dword busy, lumped columns, and the invariants of the definition against
gen.simuCarriers, gen.simuRetention, gen.simuOrigins and gen.simuIdentity.  A reference is computed once per pedigree at the largest
S and cut to the columns a case needs.  (An allele table of one label does not exist: a live set has a founder, and a founder has two.)"""
import os

import numpy as np
import pytest

from random_pedigree import random_pedigree
from test_ident_host import shapes_pedigree
from test_uniqueness_host import _rule
from uniqueness_oracle import UniqueVector, check_founders_and_children, check_lumped, check_rows, shares

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = [1, 63, 64, 65, 127, 128, 129, 200]
WAVES = 16                                   # the count kernel's workgroup: 1,024 threads
UNROLL = 4                                   # the individuals a wave has in flight
NONE = np.zeros(0, dtype=np.int64)


def _args(ped):
    return ped.ind, ped.father, ped.mother


def _ped(gen, ind, fa, mo):
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b), (np.argwhere(a != b)[:5], a[a != b][:5], b[a != b][:5])


def _check(gen, args, pro, others, S, seed, ref=None, max_share=0, **kw):
    """The two tables of one handle, computed twice, against the reference; invariant 1 on the device's tables; returns
    (alleles, autozygous, stats())."""
    if ref is None:
        ref = UniqueVector(*args, pro, others, S, seed)
    want = ref.at(S, max_share)
    h = gen.UniquenessPlan(*args, pro, others, simul_no=S, seed=seed, max_share=max_share, **kw)
    try:
        _same(h.alleles(), ref.alleles)
        _same(h.probands(), ref.ids)
        assert (h.n, h.n_pop, h.columns) == (ref.n, ref.n_pop, want[0].shape[1])
        for _ in range(2):
            h.compute()
            got = h.alleles_to_host(), h.autozygous_to_host()
            for g, w in zip(got, want):
                _same(g, w)
        check_rows(*got, S, ref.n_pop)
        st = h.stats()
        assert st["sweep_ms"] >= 0.0 and st["count_ms"] > 0.0 and st["planes"] == h.planes
        assert (st["chunk_labels"], st["chunks"], st["lds_bytes"]) == _rule(h.n_labels, kw.get("chunk_labels", 0))
        cols = kw.get("panel_cols", 0)
        pairs = min(-(-S // 128), -(-cols // 128)) if cols else -(-S // 128)
        assert (st["panel_cols"], st["panels"]) == (128 * pairs, -(-(-(-S // 128)) // pairs))
        assert st["count_bytes"] == 2 * (h.n_pop + h.n) * h.planes * 16 * -(-S // 128) * st["chunks"]
        assert st["algorithmic_bytes"] == 48 * h.planes * (2 * h.n_live - h.n_labels) * -(-S // 128)
        return got[0], got[1], st
    finally:
        h.close()


@pytest.fixture(scope="module")
def ji(gen):
    ped = gen.genealogy(gen.geneaJi)
    pro = gen.pro(ped)
    return ped, pro, UniqueVector(*_args(ped), pro, None, 200, 2024)


@pytest.mark.parametrize("S", EDGES)
def test_word_and_pair_edges(gen, ji, S):
    ped, pro, ref = ji
    _, _, st = _check(gen, _args(ped), pro, None, S, 2024, ref=ref)
    assert st["panels"] == 1 and st["chunks"] == 1


def _wide_pedigree():
    """8,000 individuals, every other one a founder or a half-founder, few generations: an allele table of a few thousand labels.  400
    probands with repeats, a non-leaf and a founder; 200 others: leaves, non-leaves, a founder and two of the probands."""
    rng = np.random.default_rng(411)
    ind, fa, mo, _ = random_pedigree(rng, 8000, p_founder=0.5, p_one_parent=0.15, p_selfing=0.03, max_back=900, max_depth=9)
    pro = rng.choice(ind[4000:], size=400, replace=False).astype(np.int64)
    parents = np.union1d(fa, mo)
    founders = ind[(fa == 0) & (mo == 0)]
    inner = parents[(parents > 0) & ~np.isin(parents, founders)]
    pro[33], pro[17], pro[5], pro[8] = pro[0], pro[0], founders[3], inner[-1]
    rest = np.setdiff1d(ind[2500:], pro)
    others = np.concatenate([rest[::27][:194], np.setdiff1d(inner, pro)[-3:], np.setdiff1d(founders, pro)[7:8], pro[1:3]]).astype(np.int64)
    return (ind, fa, mo), pro, others


@pytest.fixture(scope="module")
def wide():
    args, pro, others = _wide_pedigree()
    return args, pro, others, UniqueVector(*args, pro, others, 1000, 9)


def test_wide_case_has_the_shapes_it_claims(wide):
    (ind, fa, mo), pro, others, ref = wide
    assert 2000 <= ref.n_labels and -(-ref.n_labels // 64) >= 24 and ref.n_labels % 64 != 0 and ref.n_labels % 128 != 0 and ref.n_labels > 1216
    assert ref.n == 398 and ref.n_pop == 398 + 193 and ref.o.planes >= 11
    alleles, autozygous = ref.at(1000)
    assert alleles[:, 0].any() and alleles[:, 2:].any() and autozygous.any()


def test_forced_panels_and_chunks(gen, wide):
    """Panels of 128 and 384 simulations (S = 1,000: 8 pairs of words, the last panel of 384 ragged) crossed with chunks of 64, 128
    and 1,216 labels (dozens of chunks, the last one ragged): every handle against the reference, so the bytes are equal across all
    of them (invariant 5)."""
    args, pro, others, ref = wide
    n = ref.n_labels
    for cols, panels in ((128, 8), (384, 3)):
        for lc in (64, 128, 1216):
            _, _, st = _check(gen, args, pro, others, 1000, 9, ref=ref, panel_cols=cols, chunk_labels=lc)
            assert st["panels"] == panels and st["chunks"] == -(-n // lc) >= 2
    _check(gen, args, pro, others, 1000, 9, ref=ref)


@pytest.mark.parametrize("form", ["1", "2"])
def test_both_forms_of_the_attribute_phase(gen, wide, monkeypatch, form):
    """One atomic per lane (1) and the lanes of a wave counted by a ballot (2), picked by the hook that profiles/uniqueness_bench.py
    uses (tests/conftest.py opens the gate): the same bytes, with a column per member of the population, with 3 columns (every column
    counted by a ballot, the last one lumped) and with 6 (columns on both sides of the four that are)."""
    args, pro, others, ref = wide
    monkeypatch.setenv("GENPHI_UNIQUE_ATTRIBUTE", form)
    for max_share in (0, 3, 6):
        _check(gen, args, pro, others, 1000, 9, ref=ref, max_share=max_share, chunk_labels=128, panel_cols=384)


def _founders_and_half_founders(n_full, n_half):
    """n_full unrelated founders and n_half half-founders (children of founder 1 with an unknown mother); three children of founders 1
    and 2 (of founder 1 selfed when it is alone); a child of the last two.  2 n_full + n_half labels."""
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


@pytest.mark.parametrize("n_full,n_half", [(1, 0), (1, 1), (31, 1), (32, 0), (32, 1), (63, 1), (64, 0), (64, 1)])
def test_allele_tables_at_the_packing_edges(gen, n_full, n_half):
    """2, 3, 63, 64, 65, 127, 128 and 129 labels: a table that ends on a full dword, on a half one, on a chunk of 64 and one label past
    it, at chunk_labels 64 and 0.  Everyone is a proband."""
    ind, fa, mo = _founders_and_half_founders(n_full, n_half)
    n_labels = 2 * n_full + n_half
    ref = UniqueVector(ind, fa, mo, ind, None, 200, 3)
    assert (ref.n_labels, ref.o.planes) == (n_labels, max(1, (n_labels - 1).bit_length()))
    _, _, st = _check(gen, (ind, fa, mo), ind, None, 200, 3, ref=ref)
    assert st["chunks"] == 1
    _, _, st = _check(gen, (ind, fa, mo), ind, None, 200, 3, ref=ref, chunk_labels=64)
    assert st["chunks"] == -(-n_labels // 64)


def test_two_labels_of_one_dword_with_very_different_counts(gen):
    """1 a founder (labels 0, 1); 2 = (1, ?) a half-founder (label 2, which nobody but 2 carries); 3 a founder (labels 3, 4) with 200
    selfed children.  Labels 2 and 3 are the two halves of dword 1: a count of 1 beside counts around 150."""
    ind = np.arange(1, 204, dtype=np.int64)
    fa = np.concatenate([[0, 1, 0], np.full(200, 3)]).astype(np.int64)
    mo = np.concatenate([[0, 0, 0], np.full(200, 3)]).astype(np.int64)
    ref = UniqueVector(ind, fa, mo, ind, None, 200, 8)
    assert ref.alleles.tolist() == [[1, 0], [1, 1], [2, 1], [3, 0], [3, 1]]
    c1 = shares(ref.pop_labels, 5)
    assert np.all(c1[2] == 1) and c1[3].min() > 100 and c1[4].min() > 100
    for lc in (0, 64):
        alleles, autozygous, _ = _check(gen, (ind, fa, mo), ind, None, 200, 8, ref=ref, chunk_labels=lc)
    at = ref.ids.tolist().index(2)
    assert alleles[at, 0] == 200 and alleles[at, 1] == 200 and not autozygous[at].any()             # its own label alone; its father's with its father


@pytest.fixture(scope="module")
def clan():
    """200 individuals in few generations, closely related: the pool the proband-count tests draw from."""
    rng = np.random.default_rng(3)
    ind, fa, mo, _ = random_pedigree(rng, 200, p_founder=0.1, p_one_parent=0.05, p_selfing=0.05, max_back=20)
    return (ind, fa, mo), rng.permutation(ind)


@pytest.mark.parametrize("n_others", [0, 1, 17])
@pytest.mark.parametrize("n", [1, 2, WAVES - 1, WAVES, WAVES + 1, WAVES * UNROLL - 1, WAVES * UNROLL, WAVES * UNROLL + 1, 129])
def test_numbers_of_probands_and_others(gen, clan, n, n_others):
    """1, 2; the number of waves +- 1; the waves times the unrolling +- 1; 129: the dealing of the individuals to the waves, in the
    count phase (over n + n_others) and in the attribute phase (over n)."""
    args, order = clan
    _check(gen, args, order[:n], order[150:150 + n_others], 200, 5)


def _hub():
    """A couple with 300 children, and 300 more: the children of one of those selfed (the second shape of the carriers tests)."""
    ind = np.arange(1, 603, dtype=np.int64)
    fa = np.concatenate([[0, 0], np.full(300, 1), np.full(300, 3)]).astype(np.int64)
    mo = np.concatenate([[0, 0], np.full(300, 2), np.full(300, 3)]).astype(np.int64)
    return ind, fa, mo


@pytest.fixture(scope="module")
def hub():
    ind, fa, mo = _hub()
    return (ind, fa, mo), ind[2:], UniqueVector(ind, fa, mo, ind[2:], None, 200, 3)


def test_hub_couple_wide_counter_fields(gen, hub):
    """Every wave adds into the same four counters, the two halves of two dwords: a field passes 255 while its neighbour in the dword
    is busy too."""
    args, pro, ref = hub
    c1 = shares(ref.pop_labels, 4)
    assert c1.max() > 255 and np.all(c1.min(axis=1) > 0) and np.all((c1[0] > 255) | (c1[1] > 255) | (c1[2] > 255) | (c1[3] > 255))
    alleles, autozygous, st = _check(gen, args, pro, None, 200, 3, ref=ref)
    assert (st["levels"], st["planes"], st["columns"], st["n"], st["n_pop"]) == (3, 2, 600, 600, 600)
    assert alleles[:, 256:].any() and autozygous.any() and not alleles[:, 0].any()


@pytest.mark.parametrize("max_share", [1, 2, 37, 0])
def test_column_edges(gen, hub, max_share):
    """One column, two, 37 and all 600 (invariant 8): the cut tables are the full ones with the tail summed into the last column."""
    args, pro, ref = hub
    alleles, autozygous, st = _check(gen, args, pro, None, 200, 3, ref=ref, max_share=max_share)
    assert st["columns"] == (max_share or 600)
    full = ref.at(200)
    check_lumped(full[0], alleles)
    check_lumped(full[1], autozygous)
    if max_share == 1:
        assert np.all(alleles[:, 0] + autozygous[:, 0] == 400)


def test_half_founders_selfing_repeats_and_an_individual_in_both_lists(gen):
    ind, fa, mo = shapes_pedigree()
    pro = np.array([8, 6, 8, 5, 1, 6], dtype=np.int64)
    others = np.array([9, 7, 9, 6, 1], dtype=np.int64)                    # 6 and 1 are probands
    ref = UniqueVector(ind, fa, mo, pro, others, 2000, 4)
    assert (ref.n, ref.n_pop) == (4, 6)
    alleles, autozygous, _ = _check(gen, (ind, fa, mo), pro, others, 2000, 4, ref=ref)
    at = ref.ids.tolist().index(6)
    assert autozygous[at].sum() > 800                                    # 6 = (3, 3): selfed
    rng = np.random.default_rng(2)
    for p, o in ((np.unique(pro), np.unique(others)), (rng.permutation(pro), rng.permutation(others)), (np.concatenate([pro, pro[:3]]), others[::-1])):
        a, z, _ = _check(gen, (ind, fa, mo), p, o, 2000, 4, ref=ref)
        assert a.tobytes() == alleles.tobytes() and z.tobytes() == autozygous.tobytes()
    _check(gen, (ind, fa, mo), np.array([6], dtype=np.int64), None, 2000, 4)                         # one selfed proband alone: one column


def test_order_repeats_and_branching(gen, wide):
    (ind, fa, mo), pro, others, ref = wide
    ped = _ped(gen, ind, fa, mo)
    S = 1000
    full = gen.simuUniqueness(ped, pro, others, simulNo=S, seed=9, maxShare=0)
    _same(full.pro, ref.ids)
    assert (full.n_pop, full.simulNo, full.seed, full.lumped) == (ref.n_pop, S, 9, False)
    for g, w in zip((full.alleles, full.autozygous), ref.at(S)):
        _same(g, w)
    rng = np.random.default_rng(4)
    for p, o in ((np.unique(pro), np.unique(others)), (rng.permutation(pro), rng.permutation(others)),
                 (np.concatenate([pro, pro[:7]]), np.concatenate([others[::-1], others[:3]]))):
        r = gen.simuUniqueness(ped, p, o, simulNo=S, seed=9, maxShare=0)
        _same(r.pro, full.pro)
        assert r.alleles.tobytes() == full.alleles.tobytes() and r.autozygous.tobytes() == full.autozygous.tobytes()
    pruned = gen.branching(ped, pro=np.concatenate([pro, others]))
    assert len(pruned) < len(ped)
    r = gen.simuUniqueness(pruned, pro, others, simulNo=S, seed=9, maxShare=0)
    assert set(r.pro.tolist()) == set(full.pro.tolist())
    back = {int(x): i for i, x in enumerate(r.pro.tolist())}
    rows = [back[int(x)] for x in full.pro.tolist()]
    _same(r.alleles[rows], full.alleles)
    _same(r.autozygous[rows], full.autozygous)
    eight = gen.simuUniqueness(ped, pro, others, simulNo=S, seed=9)                                  # maxShare = 8
    assert eight.lumped and eight.mean_share is None and eight.alleles.shape == (ref.n, 8)
    check_lumped(full.alleles, eight.alleles)
    check_lumped(full.autozygous, eight.autozygous)
    _same(eight.uniqueness, full.uniqueness)


def _mid_pedigree():
    """600 individuals with founders anywhere, half-founders and selfing; 40 probands with repeats, a non-leaf and a founder (the
    recipe of tests/test_carriers_gpu.py)."""
    rng = np.random.default_rng(177)
    ind, fa, mo, _ = random_pedigree(rng, 600, p_founder=0.08, p_one_parent=0.1, p_selfing=0.03, max_back=60, max_depth=14)
    pro = rng.choice(ind[200:], size=40, replace=False).astype(np.int64)
    parents = np.union1d(fa, mo)
    founders = ind[(fa == 0) & (mo == 0)]
    inner = parents[(parents > 0) & ~np.isin(parents, founders)]
    pro[33], pro[17], pro[5], pro[8] = pro[0], pro[0], ind[0], inner[-1]
    return (ind, fa, mo), pro


@pytest.mark.parametrize("S,cols,lc", [(1000, 0, 0), (333, 128, 64)])
def test_cross_checks_with_the_sibling_sweeps(gen, S, cols, lc):
    """Invariants 2, 3 and 4, every handle on the device, same pedigree, probands and seed: no others, K = n."""
    args, pro = _mid_pedigree()
    h = gen.UniquenessPlan(*args, pro, simul_no=S, seed=77, panel_cols=cols, chunk_labels=lc)
    ids = None
    try:
        h.compute()
        ids, n = h.probands(), h.n
        assert h.columns == n == h.n_pop == 38
        alleles, autozygous = h.alleles_to_host().astype(np.int64), h.autozygous_to_host().astype(np.int64)
        table = h.alleles()
    finally:
        h.close()
    m = np.arange(1, n + 1, dtype=np.int64)
    c = gen.CarriersPlan(*args, pro, simul_no=S, seed=77, panel_cols=cols, chunk_labels=lc // 2)
    try:
        c.compute()
        _same(c.alleles(), table)
        carriers, homozygotes = c.carriers_to_host().astype(np.int64), c.homozygotes_to_host().astype(np.int64)
        assert carriers.shape[1] == n + 1
    finally:
        c.close()
    assert alleles[:, 1:].any() and autozygous.any()
    _same(alleles.sum(axis=0), m * carriers[:, 1:].sum(axis=0))                                      # 2
    assert int(autozygous.sum()) == int((homozygotes @ np.arange(n + 1, dtype=np.int64)).sum())
    g = gen.RetentionPlan(*args, pro, simul_no=S, seed=77, panel_cols=cols, chunk_labels=lc // 2)
    try:
        g.compute()
        distinct = g.distinct_to_host().astype(np.int64)
    finally:
        g.close()
    assert not (alleles.sum(axis=0) % m).any() and int((alleles.sum(axis=0) // m).sum()) == int(distinct.sum())      # 3
    o = gen.OriginsPlan(*args, ids, simul_no=S, seed=77, panel_cols=cols, chunk_labels=lc, by_proband=True)          # rows by first appearance: ids
    try:
        o.compute()
        assert o.n_grouped == n
        _same(o.by_proband_to_host().astype(np.int64).sum(axis=1), autozygous.sum(axis=1))          # 4
    finally:
        o.close()
    i = gen.IdentityPlan(*args, ids, simul_no=S, seed=77, panel_cols=cols)
    try:
        i.compute()
        _same(i.counts_to_host()[np.arange(n), np.arange(n), 0].astype(np.int64), autozygous.sum(axis=1))
    finally:
        i.close()


def test_adding_others_never_lowers_a_share(gen, wide):
    """Invariant 6, the others added in two steps, keyed by proband ID; each step against the reference first."""
    args, pro, others, ref = wide
    S = 1000
    steps = []
    for o in (NONE, others[:60], others):
        r = ref if len(o) == len(others) else UniqueVector(*args, pro, o, S, 9)
        a, z, _ = _check(gen, args, pro, o, S, 9, ref=r)
        at = {int(x): k for k, x in enumerate(r.ids.tolist())}
        rows = [at[int(x)] for x in ref.ids.tolist()]
        steps.append((a[rows].astype(np.int64), z[rows].astype(np.int64)))
    assert steps[0][0].shape[1] < steps[1][0].shape[1] < steps[2][0].shape[1]
    lowered = 0
    for before, after in zip(steps[:2], steps[1:]):
        for narrow, widened in zip(before, after):
            pad = np.zeros(widened.shape, dtype=np.int64)
            pad[:, : narrow.shape[1]] = narrow
            assert np.all(np.cumsum(widened, axis=1) <= np.cumsum(pad, axis=1))
            lowered += int(np.any(np.cumsum(widened, axis=1) < np.cumsum(pad, axis=1)))
    assert lowered >= 2


def test_lone_founders_and_children_of_the_population(gen, wide):
    """Invariant 7 on a hand-made pedigree: 1, 2 founders; 3 = (1, 2); 4 a founder with no descendant; 5 a founder whose child 6 is
    neither listed nor an ancestor of anyone listed.  Probands 3, 4, 5; others 1, 2, then also with max_share = 2 and 1.  Then on the
    wide case."""
    ind = np.arange(1, 7, dtype=np.int64)
    fa = np.array([0, 0, 1, 0, 0, 5], dtype=np.int64)
    mo = np.array([0, 0, 2, 0, 0, 0], dtype=np.int64)
    S = 500
    pro, others = np.array([3, 4, 5], dtype=np.int64), np.array([1, 2], dtype=np.int64)
    ref = UniqueVector(ind, fa, mo, pro, others, S, 6)
    alleles, autozygous, _ = _check(gen, (ind, fa, mo), pro, others, S, 6, ref=ref)
    assert check_founders_and_children(alleles, autozygous, ref.ids, ref.pop_ids, ind, fa, mo, S) == (2, 1)
    at = ref.ids.tolist()
    assert alleles[at.index(4)].tolist() == [2 * S, 0, 0, 0, 0] and alleles[at.index(3)].tolist() == [0, 2 * S, 0, 0, 0] and not autozygous.any()
    two, two_z, _ = _check(gen, (ind, fa, mo), pro, others, S, 6, ref=ref, max_share=2)
    assert check_founders_and_children(two, two_z, ref.ids, ref.pop_ids, ind, fa, mo, S) == (2, 1)
    one, _, _ = _check(gen, (ind, fa, mo), pro, others, S, 6, ref=ref, max_share=1)
    assert one.tolist() == [[2 * S]] * 3                                                             # K = 1: everything in the one column
    alone, _, _ = _check(gen, (ind, fa, mo), np.array([4], dtype=np.int64), np.array([1, 3, 5], dtype=np.int64), S, 6)
    assert alone.tolist() == [[2 * S, 0, 0, 0]]
    (wi, wf, wm), wpro, wothers, wref = wide
    a, z = wref.at(1000)
    lone, children = check_founders_and_children(a, z, wref.ids, wref.pop_ids, wi, wf, wm, 1000)
    assert lone >= 1


def test_both_halves_of_the_seed(gen, clan):
    """A seed with only its low half set and one with only its high half set each match the reference, and differ."""
    args, order = clan
    pro, others = order[:30], order[100:110]
    low, _, _ = _check(gen, args, pro, others, 200, 0x12345678)
    high, _, _ = _check(gen, args, pro, others, 200, 0x12345678 << 32)
    assert not np.array_equal(low, high)


def test_ids_above_2_to_the_32(gen):
    ind, fa, mo = shapes_pedigree()

    def big(x):
        return np.where(x > 0, x * (1 << 33) + 5, 0).astype(np.int64)

    args = (big(ind), big(fa), big(mo))
    pro, others = big(np.array([8, 6, 5])), big(np.array([9, 7]))
    ref = UniqueVector(*args, pro, others, 1000, 12)
    alleles, _, _ = _check(gen, args, pro, others, 1000, 12, ref=ref)
    assert ref.ids.min() > 2**32 and alleles[:, 1:].any()
    small = UniqueVector(ind, fa, mo, [8, 6, 5], [9, 7], 1000, 12)
    assert not np.array_equal(small.at(1000)[0], alleles)                # the ID keys the random stream, both halves of it


@pytest.mark.parametrize("name", ["geneaJi", "genea140"])
def test_simuUniqueness_end_to_end(gen, name):
    ped = gen.genealogy(getattr(gen, name))
    if name == "geneaJi":
        S, pro, others = 5000, gen.pro(ped), NONE
        r = gen.simuUniqueness(ped, simulNo=S, seed=21)
    else:
        S = 1000
        pop = gen._pop(os.path.join(ROOT, "tests", "golden", "pop140.csv"))
        pro = np.array(sorted(k for k, v in pop.items() if v == "Saguenay"), dtype=np.int64)
        others = np.array(sorted(k for k, v in pop.items() if v != "Saguenay"), dtype=np.int64)
        assert len(pro) == 22 and len(others) == 118
        r = gen.simuUniqueness(ped, pro, others, simulNo=S, seed=21)
    n, n_pop = len(pro), len(pro) + len(others)
    K = min(8, n_pop)
    assert np.array_equal(np.sort(r.pro), np.unique(pro)) and r.n_pop == n_pop and (r.simulNo, r.seed) == (S, 21)
    assert r.alleles.shape == r.autozygous.shape == r.copies.shape == (n, K)
    assert r.alleles.dtype == r.autozygous.dtype == np.int32 and r.copies.dtype == np.int64
    check_rows(r.alleles, r.autozygous, S, n_pop)
    assert r.uniqueness.dtype == r.at_risk.dtype == np.float64 and np.all((r.uniqueness >= 0.0) & (r.uniqueness <= 1.0)) and np.all((r.at_risk >= 0.0) & (r.at_risk <= 2.0))
    assert r.share_hist.shape == (n, K) and np.all(np.abs(r.share_hist.sum(axis=1) - 1.0) <= 1e-12)
    assert r.lumped == (K < n_pop) and (r.mean_share is None) == r.lumped
    rank = r.ranking(5)
    assert len(rank) == min(5, n) and np.all(np.diff(r.uniqueness[rank]) <= 0)
    h = gen.UniquenessPlan(*_args(ped), pro, others, simul_no=S, seed=21, max_share=8)
    try:
        for _ in range(2):
            h.compute()
            _same(h.alleles_to_host(), r.alleles)
            _same(h.autozygous_to_host(), r.autozygous)
        _same(h.probands(), r.pro)
    finally:
        h.close()
    if name == "geneaJi":
        ref = UniqueVector(*_args(ped), pro, others, S, 21)
        for g, w in zip((r.alleles, r.autozygous), ref.at(S, 8)):
            _same(g, w)
    else:
        assert np.any(r.alleles[:, 0] > 0) and np.any(r.alleles[:, 1:] > 0)
    fresh = gen.simuUniqueness(ped, pro, others, simulNo=256)
    again = gen.simuUniqueness(ped, pro, others, simulNo=256)
    assert fresh.seed != again.seed
    replay = gen.simuUniqueness(ped, pro, others, simulNo=256, seed=fresh.seed)
    _same(replay.alleles, fresh.alleles)
    _same(replay.autozygous, fresh.autozygous)
