"""gen.implex on the CPU: the two oracles of tests/implex_oracle.py against each other and against the pins (a plain breadth-first
search over the bundled CSVs); the host-only parts of the library: planning without a GPU, the number of generations, the union
frontier |U_g| per generation, argument errors, exports."""
import numpy as np
import pytest

from implex_oracle import implex_frontier, implex_literal, ind_matrix, mean_column
from random_pedigree import random_pedigree
from test_occ_reference import QUIRK_PRO, doubling_chain, quirk_pedigree

# geneaJi, pro = [1, 2, 29], G = 8
JI_COUNTS = np.array([[1, 2, 4, 5, 5, 4, 4, 2], [1, 2, 4, 5, 5, 4, 4, 2], [1, 2, 4, 4, 2, 2, 2, 0]], dtype=np.int64)
JI_NEW = np.array([[1, 2, 4, 5, 5, 2, 2, 0], [1, 2, 4, 5, 5, 2, 2, 0], [1, 2, 4, 4, 2, 2, 0, 0]], dtype=np.int64)
JI_MEAN = [100.0, 100.0, 100.0, 58.333333333333336, 25.0, 10.416666666666666, 5.208333333333333, 1.0416666666666667]
# genea140, 140 probands, G = 18
G140_TOTALS = [140, 280, 560, 1092, 2112, 3933, 7114, 12857, 22883, 38233, 57607, 69361, 53387, 27079, 9058, 2034, 344, 32]
G140_NEW_TOTALS = [140, 280, 560, 1092, 2106, 3894, 6966, 12391, 21609, 34594, 48477, 51862, 30776, 10599, 1905, 180, 10, 0]
G140_PRO = 217891
G140_PRO_COUNTS = [1, 2, 4, 8, 16, 32, 62, 123, 211, 341, 515, 508, 226, 64, 6, 0, 0, 0]
G140_PRO_NEW = [1, 2, 4, 8, 16, 32, 62, 120, 202, 305, 434, 344, 84, 8, 0, 0, 0, 0]


def _args(ped):
    return ped.ind, ped.father, ped.mother


def both_oracles(ind, father, mother, pro, only_new=False):
    """(counts, rows) of the two oracles, which must agree."""
    lit, rows_lit = implex_literal(ind, father, mother, pro, only_new)
    fro, rows_fro = implex_frontier(ind, father, mother, pro, only_new)
    assert lit.shape == fro.shape and lit.dtype == fro.dtype == np.int64
    assert np.array_equal(lit, fro)
    assert rows_lit == rows_fro
    return fro, rows_fro


def mixed_probands(rng, ind, n):
    """n proband IDs drawn from anywhere in the pedigree (founders, non-leaves, ancestors of one another), some listed twice."""
    pro = rng.choice(ind, size=n, replace=True)
    if n >= 3:
        pro[n - 1] = pro[0]
    return pro.astype(np.int64)


def random_case(seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(2, 401))
    ind, fa, mo, _ = random_pedigree(rng, n, p_founder=float(rng.uniform(0.02, 0.4)), p_one_parent=float(rng.uniform(0.0, 0.3)),
                                     p_selfing=0.05, max_back=int(rng.integers(2, 60)), max_depth=int(rng.integers(2, 40)))
    return ind, fa, mo, mixed_probands(rng, ind, int(rng.integers(1, 90)))


def _check_plan(gen, ind, fa, mo, pro):
    for only_new in (False, True):
        counts, rows = both_oracles(ind, fa, mo, pro, only_new)
        h = gen.ImplexPlan(ind, fa, mo, pro, only_new=only_new)
        try:
            assert h.generations == counts.shape[1] == len(rows)
            assert h.shape == counts.shape
            got = h.rows_per_generation()
            assert got.dtype == np.int64 and got.tolist() == rows
        finally:
            h.close()
    return counts.shape[1]


def test_oracles_reproduce_the_geneaJi_pins(gen):
    ped = gen.genealogy(gen.geneaJi)
    pro = gen.pro(ped)
    assert list(pro) == [1, 2, 29]
    counts, rows = both_oracles(*_args(ped), pro)
    assert np.array_equal(counts, JI_COUNTS)
    assert np.array_equal(both_oracles(*_args(ped), pro, only_new=True)[0], JI_NEW)
    assert mean_column(counts).ravel().tolist() == JI_MEAN
    assert ind_matrix(counts).shape == (8, 3) and ind_matrix(counts)[3].tolist() == [62.5, 62.5, 50.0]
    assert rows[0] == 3 and len(rows) == 8


def test_oracles_reproduce_the_genea140_pins(gen):
    ped = gen.genealogy(gen.genea140)
    pro = gen.pro(ped)
    assert len(pro) == 140
    counts, rows = both_oracles(*_args(ped), pro)
    new, rows_new = both_oracles(*_args(ped), pro, only_new=True)
    assert counts.shape == new.shape == (140, 18) and rows == rows_new
    assert counts.sum(axis=0).tolist() == G140_TOTALS
    assert new.sum(axis=0).tolist() == G140_NEW_TOTALS
    i = pro.tolist().index(G140_PRO)
    assert counts[i].tolist() == G140_PRO_COUNTS
    assert new[i].tolist() == G140_PRO_NEW and int(new[i, 1:].sum()) == 1621
    assert np.all(new <= counts)


def test_plan_on_the_bundled_pedigrees(gen):
    for path, G in ((gen.geneaJi, 8), (gen.genea140, 18)):
        ped = gen.genealogy(path)
        assert _check_plan(gen, *_args(ped), gen.pro(ped)) == G == gen.depth(ped)


def test_plan_on_the_quirk_pedigree(gen):
    ped = quirk_pedigree(gen)
    assert _check_plan(gen, *_args(ped), np.array(QUIRK_PRO)) == 5
    assert _check_plan(gen, *_args(ped), np.array([10, 1, 10])) == 1           # founders only
    h = gen.ImplexPlan(*_args(ped), QUIRK_PRO)
    c = gen.CompletenessPlan(*_args(ped), QUIRK_PRO)
    try:
        assert h.generations == c.generations
        # U_0 = {12, 8, 3, 10, 1}, U_1 = {8, 9, 6, 7, 1, 2}, U_2 = {6, 7, 4, 3, 5}, U_3 = {3, 5, 4, 1, 2}, U_4 = {1, 2}
        assert h.rows_per_generation().tolist() == [5, 6, 5, 5, 2]
    finally:
        h.close()
        c.close()


@pytest.mark.parametrize("block", range(8))
def test_plan_on_random_pedigrees(gen, block):
    """200 draws: founders anywhere, one-parent members, selfing; mixed, duplicated, non-leaf proband lists."""
    for seed in range(25 * block, 25 * block + 25):
        ind, fa, mo, pro = random_case(seed)
        G = _check_plan(gen, ind, fa, mo, pro)
        c = gen.CompletenessPlan(ind, fa, mo, pro)
        try:
            assert c.generations == G
        finally:
            c.close()


def test_argument_errors_without_a_device(gen):
    ped = gen.genealogy(gen.geneaJi)
    with pytest.raises(KeyError):
        gen.ImplexPlan(*_args(ped), [1, 999])
    with pytest.raises(KeyError):
        gen.implex(ped, [1, 999])
    with pytest.raises(ValueError):
        gen.implex(ped, [])
    for bad in ("ALL", "mean", None):
        with pytest.raises(ValueError):
            gen.implex(ped, type=bad)
    for bad in ([8], [-1], [0, 3, 8]):
        with pytest.raises(IndexError):
            gen.implex(ped, genNo=bad)
        with pytest.raises(IndexError):
            gen.implex(ped, genNo=bad, type="IND", onlyNewAnc=True)


def test_depth_limit(gen):
    ind, fa, mo = doubling_chain(63)
    h = gen.ImplexPlan(ind, fa, mo, [125, 126])
    try:
        assert h.generations == 63
        assert h.rows_per_generation().tolist() == [2] * 63
    finally:
        h.close()
    ind, fa, mo = doubling_chain(64)
    with pytest.raises(ValueError, match="63 generations above the probands"):
        gen.ImplexPlan(ind, fa, mo, [127])
    h = gen.ImplexPlan(ind, fa, mo, [125, 3])                                  # the limit is about the listed probands
    h.close()


def test_exports(gen):
    assert gen.ImplexPlan is gen._capi.ImplexPlan
    L = gen._capi.lib()
    for name in gen._capi.EXPORTED_SYMBOLS:
        if name.startswith("genphi_implex_"):
            assert hasattr(L, name)
    assert sum(name.startswith("genphi_implex_") for name in gen._capi.EXPORTED_SYMBOLS) == 9
