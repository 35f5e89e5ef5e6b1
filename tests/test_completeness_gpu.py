"""gen.completeness on the MI355X against tests/completeness_oracle.py: every entry of "IND", of the counts and of the totals is
compared with np.array_equal; "MEAN" with np.array_equal inside its exact range (25 totals[g] < 2^53 for every g) and within 2 ulp
of the exact rational mean beyond it."""
from fractions import Fraction

import numpy as np
import pytest

from completeness_oracle import completeness_exact, completeness_literal, mean_fraction
from test_completeness_reference import G140_TOTALS, JI_IND, JI_MEAN_0_4_6, QUIRK_COUNTS, QUIRK_IND, QUIRK_MEAN
from test_gc_gpu import _mixed_lists, _one_parent_synth
from test_mrca_gpu import cfg3  # noqa: F401  (a fixture)
from test_occ_reference import QUIRK_PRO, doubling_chain, quirk_pedigree

pytestmark = pytest.mark.gpu


def _args(ped):
    return ped.ind, ped.father, ped.mother


def _ped(gen, ind, fa, mo, sex=None, sort=True):
    sex = np.ones(len(ind), dtype=np.int64) if sex is None else sex
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}, sort=sort)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b), np.argwhere(a != b)[:5]


def _in_exact_range(counts):
    return all(25 * sum(int(v) for v in counts[:, g]) < 2 ** 53 for g in range(counts.shape[1]))


def _mean_in_range(counts):
    """The reference's mean where every partial sum is exact: any order gives it, here exact rationals rounded once."""
    assert _in_exact_range(counts)
    return np.array([[float(f)] for f in mean_fraction(counts)])


def _check_everything(gen, ped, pro, exact=None):
    """IND, counts, totals and MEAN of one pedigree and proband list against the exact oracle (all entries)."""
    counts, ind_matrix = exact if exact is not None else completeness_exact(*_args(ped), pro)
    _same(gen.completeness(ped, pro, type="IND"), ind_matrix)
    h = gen.CompletenessPlan(*_args(ped), pro)
    try:
        h.compute()
        _same(h.counts(), counts)
        _same(h.result_to_host(), np.ascontiguousarray(ind_matrix.T))
        _same(h.totals(), counts.sum(axis=0, dtype=np.int64))
        _same(h.totals(), counts.sum(axis=0, dtype=np.int64))          # asked again: the same
        _same(h.result_to_host(), np.ascontiguousarray(ind_matrix.T))  # the column sums left the resident result alone
        st = h.stats()
    finally:
        h.close()
    _same(gen.completeness(ped, pro), _mean_in_range(counts))
    return st


def test_geneaJi_pins(gen):
    ped = gen.genealogy(gen.geneaJi)
    ind_matrix = gen.completeness(ped, type="IND")
    assert ind_matrix[7, 0] == 3.125                                   # test/runtests.jl:68
    _same(ind_matrix, JI_IND)
    _same(gen.completeness(ped, genNo=[0, 4, 6]), JI_MEAN_0_4_6)       # :69
    _same(gen.completeness(ped), completeness_literal(*_args(ped), gen.pro(ped)))
    _same(gen.completeness(ped, genNo=[6, 0, 6, 7], type="IND"), JI_IND[[6, 0, 6, 7]])
    assert ind_matrix.shape[0] == gen.depth(ped) == 8
    assert not ind_matrix.flags["C_CONTIGUOUS"] and ind_matrix.T.flags["C_CONTIGUOUS"]      # a view of the row-major result


def test_quirk_pedigree(gen):
    ped = quirk_pedigree(gen)
    _same(gen.completeness(ped, QUIRK_PRO, type="IND"), QUIRK_IND)
    _same(gen.completeness(ped, QUIRK_PRO), QUIRK_MEAN)
    _same(gen.completeness(ped, QUIRK_PRO, genNo=[4, 0, 4]), QUIRK_MEAN[[4, 0, 4]])
    _same(gen.completeness(ped, [10, 1, 10], type="IND"), np.full((1, 3), 100.0))           # founders only: one launch, no slots
    _same(gen.completeness(ped, [10]), np.full((1, 1), 100.0))
    h = gen.CompletenessPlan(*_args(ped), QUIRK_PRO)
    try:
        h.compute()
        _same(h.counts(), QUIRK_COUNTS)
        _same(h.totals(), QUIRK_COUNTS.sum(axis=0))
    finally:
        h.close()


def test_genea140_default_arguments(gen):
    ped = gen.genealogy(gen.genea140)
    pro = gen.pro(ped)
    exact = completeness_exact(*_args(ped), pro)
    _check_everything(gen, ped, pro, exact)
    ind_matrix = gen.completeness(ped, type="IND")
    assert ind_matrix.shape == (18, 140) and ind_matrix.shape[0] == gen.depth(ped)
    for totals_only in (False, True):
        h = gen.CompletenessPlan(*_args(ped), pro, totals_only=totals_only)
        try:
            h.compute()
            assert [int(v) for v in h.totals()] == G140_TOTALS
            if totals_only:
                with pytest.raises(ValueError):
                    h.result_to_host()
        finally:
            h.close()
    _same(gen.completeness(ped), completeness_literal(*_args(ped), pro))                     # the literal sequential sum
    _same(gen.completeness(ped, genNo=[17, 3]), completeness_literal(*_args(ped), pro, genNo=[17, 3]))


def test_genea140_mixed_probands(gen):
    """A subset in shuffled order with repeats, non-leaf and founder probands."""
    ped = gen.genealogy(gen.genea140)
    pro, _ = _mixed_lists(ped, gen, np.random.default_rng(11), 13)
    assert len(set(pro.tolist())) < len(pro) and not set(pro.tolist()) <= set(gen.pro(ped).tolist())
    _check_everything(gen, ped, pro)


def test_cfg3_all_entries(gen, cfg3):  # noqa: F811
    ped, pro = cfg3
    exact = completeness_exact(*_args(ped), pro)
    st = _check_everything(gen, ped, pro, exact)
    assert st["launches"] == exact[0].shape[1] == 20


def test_skip_generations_one_parent_members_all_entries(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(100_000, 10_000, 20, skip_permille=50)
    fa, mo = fa.copy(), mo.copy()
    k = np.arange(len(ind))
    mo[(k % 13 == 5) & (fa != 0)] = 0
    fa[(k % 17 == 3) & (mo != 0)] = 0
    ped = _ped(gen, ind, fa, mo, sex)
    st = _check_everything(gen, ped, pro)
    assert st["peak_slots"] < len(gen.ancestor(ped, pro))


def test_unsorted_pedigree(gen):
    """sort=False: the rank order is the file order (generation by generation, late founders in the middle of the file)."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(6000, 500, 12, skip_permille=30)
    ped = _ped(gen, ind, fa, mo, sex, sort=False)
    assert np.array_equal(ped.ind, ind) and not np.array_equal(_ped(gen, ind, fa, mo, sex).ind, ind)
    _check_everything(gen, ped, pro[::-1])


def test_overlapping_generations_reuse_slots(gen):
    """Members dragged across several cuts, slots freed and handed out again: fewer slots than computed rows."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = _one_parent_synth(synth)
    ped = _ped(gen, ind, fa, mo, sex)
    for probands in (pro, _mixed_lists(ped, gen, np.random.default_rng(5), 21)[0]):
        st = _check_everything(gen, ped, probands)
        computed_rows = len(gen.ancestor(ped, probands))               # every strict ancestor of a proband owns one slot row
        assert 0 < st["peak_slots"] < computed_rows


def test_doubling_chain_reaches_the_top_of_int64(gen):
    ind, fa, mo = doubling_chain(63)
    ped = _ped(gen, ind, fa, mo)
    _same(gen.completeness(ped, [126], type="IND"), np.full((63, 1), 100.0))
    _same(gen.completeness(ped, [126]), np.full((63, 1), 100.0))       # one proband: the totals are its counts
    h = gen.CompletenessPlan(*_args(ped), [126, 125])
    try:
        h.compute()
        counts = h.counts()
        _same(counts, np.array([[2 ** g for g in range(63)]] * 2, dtype=np.int64))
        assert int(counts[0, 62]) == 2 ** 62
        _same(h.result_to_host(), np.full((2, 63), 100.0))
        with pytest.raises(ValueError):
            h.totals()                                                 # 62 + 1 bits
    finally:
        h.close()
    with pytest.raises(ValueError):
        gen.CompletenessPlan(*_args(ped), [126, 125], totals_only=True)
    _same(gen.completeness(ped, [126, 125]), np.full((63, 1), 100.0))  # "MEAN" by the sequential sum of "IND"


def ring_chain(generations, width=4, cut_every=3):
    """A doubling chain `width` wide: member j of generation g has father j and mother j + 1 (mod width) of generation g - 1, so
    without gaps every member has 2^k ascending paths of k meioses.  Every `cut_every`-th generation one member (a different
    position each time) loses its mother: a removed link takes away the paths that ran through it, an eighth or so of them, and
    the links removed at different depths overlap, so the deep counts stay close to 2^k and have dense bit patterns.  (In the
    chain two wide of doubling_chain the full generations between two gaps make the counts products 2^a 3^r, and 25 * 3^r
    needs r >= 31 gaps, 62 generations, to leave Float64: out of reach of a totals handle with three probands.)"""
    n = width * generations
    ind = np.arange(1, n + 1)
    fa, mo = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for g in range(1, generations):
        for j in range(width):
            fa[g * width + j] = (g - 1) * width + j + 1
            mo[g * width + j] = (g - 1) * width + (j + 1) % width + 1
        if g % cut_every == 0:
            mo[g * width + (g // cut_every) % width] = 0
    return ind, fa, mo


def test_mean_beyond_its_exact_range_is_within_2_ulp(gen):
    """60 generations, links removed at 19 depths, 5 probands of the last two generations.  The bound of 2 ulp is derived
    (include/genphi.h: the conversion of the total, x 100 and / n round by half an ulp each; / 2^g is exact), not measured."""
    ind, fa, mo = ring_chain(60)
    ped = _ped(gen, ind, fa, mo)
    pro = [240, 239, 238, 235, 234]
    counts, ind_matrix = completeness_exact(*_args(ped), pro)
    n, G = counts.shape
    assert G == 60 and n >= 3
    totals = [sum(int(v) for v in counts[:, g]) for g in range(G)]
    assert any(25 * t >= 2 ** 53 for t in totals)                                                   # outside the exact range
    assert any(int(float(25 * int(v))) != 25 * int(v) for v in counts.ravel())                      # an entry that Float64 rounds
    _same(gen.completeness(ped, pro, type="IND"), ind_matrix)
    h = gen.CompletenessPlan(*_args(ped), pro, totals_only=True)                                    # 59 + 3 bits: the totals fit
    try:
        h.compute()
        assert [int(v) for v in h.totals()] == totals
    finally:
        h.close()
    mean = gen.completeness(ped, pro)
    assert mean.shape == (G, 1) and mean.dtype == np.float64
    worst = 0.0
    for g in range(G):
        exact = Fraction(totals[g] * 100, (2 ** g) * n)
        err = abs(Fraction(float(mean[g, 0])) - exact)
        ulp = Fraction(float(np.spacing(mean[g, 0])))
        worst = max(worst, float(err / ulp))
        assert err <= 2 * ulp, (g, float(err / ulp))
    print("gen.completeness MEAN beyond the exact range: worst error %.3f ulp" % worst)


def test_stats(gen):
    ped = gen.genealogy(gen.genea140)
    pro, _ = _mixed_lists(ped, gen, np.random.default_rng(2), 13)
    anc = set(gen.ancestor(ped, pro).tolist())                        # the members with a slot row (strict ancestors of a proband)
    n_par = dict(zip(ped.ind.tolist(), ((ped.father != 0).astype(int) + (ped.mother != 0)).tolist()))
    written = len(anc)
    read = sum(n_par[a] for a in anc) + sum(1 if int(p) in anc else n_par[int(p)] for p in pro)     # a proband in a slot is copied
    for totals_only in (False, True):
        h = gen.CompletenessPlan(*_args(ped), pro, totals_only=totals_only)
        try:
            G = h.generations
            h.compute()
            st = h.stats()
        finally:
            h.close()
        result = 8 * G if totals_only else 16 * G * len(pro)          # totals; counts and percentages
        assert st["sweep_ms"] > 0
        assert st["algorithmic_bytes"] == 8 * G * (read + written) + result
        assert st["launches"] == G                                    # one list per cut, none of them empty
        assert st["row_entries"] == (G + 7) // 8 * 8 and 0 < st["peak_slots"] <= written
