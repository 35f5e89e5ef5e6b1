"""gen.implex on the MI355X against tests/implex_oracle.py: every entry of the counts, of "IND", of the totals and of "MEAN" is
compared with np.array_equal ("MEAN" against the exact rational mean rounded once); every handle is computed twice with equal
bits.  Shapes are the smallest at which each part of csrc/implex.hip can go wrong: proband word edges, child lists longer than
a wave, overlapping generations, ragged panels, several panels per launch, every lanes-per-row form of the step kernel (pinned
through stats()), the depth limit."""
import numpy as np
import pytest

from implex_oracle import ind_matrix, mean_column
from random_pedigree import random_pedigree
from test_gc_gpu import _one_parent_synth
from test_implex_host import (G140_NEW_TOTALS, G140_PRO, G140_PRO_COUNTS, G140_PRO_NEW, G140_TOTALS, JI_COUNTS, JI_MEAN, JI_NEW,
                              both_oracles)
from test_occ_reference import doubling_chain

pytestmark = pytest.mark.gpu


def _args(ped):
    return ped.ind, ped.father, ped.mother


def _ped(gen, ind, fa, mo):
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b), np.argwhere(a != b)[:5]


def _check_handle(gen, ind, fa, mo, pro, only_new, counts):
    """counts, percentages and totals of one handle, computed twice; returns its stats."""
    h = gen.ImplexPlan(ind, fa, mo, pro, only_new=only_new)
    try:
        for _ in range(2):
            h.compute()
            _same(h.counts(), counts)
            _same(h.result_to_host(), np.ascontiguousarray(ind_matrix(counts).T))
            _same(h.totals(), counts.sum(axis=0, dtype=np.int64))
            _same(h.totals(), counts.sum(axis=0, dtype=np.int64))          # asked again: the same
        return h.stats()
    finally:
        h.close()


def _check_everything(gen, ped, pro, oracles=None):
    """Both modes of one pedigree and proband list against the oracles: the handle and the public function."""
    pro = np.asarray(pro, dtype=np.int64)
    stats = []
    for only_new in (False, True):
        counts = oracles[only_new] if oracles is not None else both_oracles(*_args(ped), pro, only_new)[0]
        stats.append(_check_handle(gen, *_args(ped), pro, only_new, counts))
        ind = gen.implex(ped, pro, type="IND", onlyNewAnc=only_new)
        _same(ind, ind_matrix(counts))
        assert ind.T.flags["C_CONTIGUOUS"] and (ind.shape[0] == 1 or ind.shape[1] == 1 or not ind.flags["C_CONTIGUOUS"])
        _same(gen.implex(ped, pro, onlyNewAnc=only_new), mean_column(counts))
    return stats


@pytest.fixture(scope="module")
def word_edge_case(gen):
    """About 2,000 individuals with founders anywhere, one-parent members and selfing; 129 probands: the first is the child of
    the second (a proband that is an ancestor of another), then founders, non-leaves and duplicates."""
    rng = np.random.default_rng(77)
    ind, fa, mo, _ = random_pedigree(rng, 2000, p_founder=0.08, p_one_parent=0.1, p_selfing=0.02, max_back=300, max_depth=14)
    child = int(np.flatnonzero(fa != 0)[-1])
    pro = rng.choice(ind, size=129, replace=True).astype(np.int64)
    pro[0], pro[1] = ind[child], fa[child]
    pro[2] = ind[np.flatnonzero((fa == 0) & (mo == 0))[3]]                # a founder
    pro[62], pro[63], pro[64], pro[128] = pro[0], pro[1], pro[0], pro[5]   # duplicates across the word edges
    return _ped(gen, ind, fa, mo), pro


@pytest.fixture(scope="module")
def synth400(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = _one_parent_synth(synth)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pro = np.asarray(pro, dtype=np.int64)
    assert len(ind) == 4000 and len(pro) == 400
    return ped, pro, {m: both_oracles(*_args(ped), pro, m)[0] for m in (False, True)}


def test_geneaJi_pins(gen):
    ped = gen.genealogy(gen.geneaJi)
    _check_everything(gen, ped, gen.pro(ped), {False: JI_COUNTS, True: JI_NEW})
    assert gen.implex(ped).ravel().tolist() == JI_MEAN
    ind = gen.implex(ped, type="IND")
    assert ind.shape == (8, 3) and not ind.flags["C_CONTIGUOUS"] and ind.T.flags["C_CONTIGUOUS"]      # a view of the row-major result
    _same(gen.implex(ped, genNo=[6, 0, 6, 7], type="IND"), ind_matrix(JI_COUNTS)[[6, 0, 6, 7]])
    _same(gen.implex(ped, genNo=[7, 7, 3], onlyNewAnc=True), mean_column(JI_NEW)[[7, 7, 3]])


def test_genea140_pins(gen):
    ped = gen.genealogy(gen.genea140)
    pro = gen.pro(ped)
    oracles = {m: both_oracles(*_args(ped), pro, m)[0] for m in (False, True)}
    _check_everything(gen, ped, pro, oracles)
    i = pro.tolist().index(G140_PRO)
    for only_new, totals, row in ((False, G140_TOTALS, G140_PRO_COUNTS), (True, G140_NEW_TOTALS, G140_PRO_NEW)):
        h = gen.ImplexPlan(*_args(ped), pro, only_new=only_new)
        try:
            h.compute()
            assert h.totals().tolist() == totals and h.counts()[i].tolist() == row
        finally:
            h.close()
    _same(gen.implex(ped, genNo=[17, 3, 17]), mean_column(oracles[False])[[17, 3, 17]])


@pytest.mark.parametrize("n_pro", [1, 63, 64, 65, 128, 129])
def test_proband_word_edges(gen, word_edge_case, n_pro):
    ped, pro = word_edge_case
    _check_everything(gen, ped, pro[:n_pro])


def test_hub_child_lists(gen):
    """One couple with 300 children and one with 65, all probands: child lists longer than a wave and than the unrolled part of
    the loop; the hub parents have parents of their own, one of them shared between the couples."""
    ind = np.arange(1, 9 + 365, dtype=np.int64)
    fa, mo = np.zeros(len(ind), dtype=np.int64), np.zeros(len(ind), dtype=np.int64)
    fa[4], mo[4] = 1, 2            # 5 = (1, 2)
    fa[5], mo[5] = 3, 4            # 6 = (3, 4)
    fa[7], mo[7] = 1, 2            # 8 = (1, 2); 7 is a founder
    fa[8:308], mo[8:308] = 5, 6    # 300 children of (5, 6)
    fa[308:], mo[308:] = 7, 8      # 65 children of (7, 8)
    ped = _ped(gen, ind, fa, mo)
    pro = np.concatenate([ind[8:], [5, 9]])
    st = _check_everything(gen, ped, pro)
    assert st[0]["generations"] == 3 and st[0]["peak_rows"] == 366


def test_one_parent_synth(gen, synth400):
    ped, pro, oracles = synth400
    st = _check_everything(gen, ped, pro, oracles)
    assert st[0]["panels"] == 1 and st[0]["panel_cols"] == 448              # the default panel: the words the probands need


# panel columns -> lanes per row of the step kernel (one 16-byte pair per lane; 16,384 columns: two pairs per lane)
FORMS = [(64, 1), (128, 1), (256, 2), (512, 4), (1024, 8), (2048, 16), (4096, 32), (8192, 64), (16384, 64)]


@pytest.mark.parametrize("panel,lpr", FORMS)
def test_every_step_form(gen, synth400, monkeypatch, panel, lpr):
    ped, pro, oracles = synth400
    monkeypatch.setenv("GENPHI_IMPLEX_PANEL", str(panel))
    for only_new in (False, True):
        st = _check_handle(gen, *_args(ped), pro, only_new, oracles[only_new])
        assert st["lanes_per_row"] == lpr and st["panel_cols"] == panel and st["panels"] == -(-400 // panel)


@pytest.mark.parametrize("panel,per_launch", [(64, 1), (64, 3), (64, 7), (128, 2), (100, 0)])
def test_forced_panels(gen, synth400, monkeypatch, panel, per_launch):
    """400 probands in panels of 64 (7 panels, the last of 16 columns) and 128 (4, the last of 16), one, some and all per launch;
    a width that is no multiple of 64 is rounded up."""
    ped, pro, oracles = synth400
    monkeypatch.setenv("GENPHI_IMPLEX_PANEL", str(panel))
    if per_launch:
        monkeypatch.setenv("GENPHI_IMPLEX_PANELS_PER_LAUNCH", str(per_launch))
    cols = -(-panel // 64) * 64
    for only_new in (False, True):
        st = _check_handle(gen, *_args(ped), pro, only_new, oracles[only_new])
        assert st["panel_cols"] == cols and st["panels"] == -(-400 // cols)
        assert st["algorithmic_bytes"] > 0 and st["sweep_ms"] > 0


def test_depth_limit(gen):
    ind, fa, mo = doubling_chain(63)
    ped = _ped(gen, ind, fa, mo)
    for only_new in (False, True):
        counts = both_oracles(ind, fa, mo, [125, 126, 125], only_new)[0]
        assert counts.shape == (3, 63) and np.all(counts[:, 1:] == 2) and np.all(counts[:, 0] == 1)
        _check_handle(gen, ind, fa, mo, [125, 126, 125], only_new, counts)
    ind_m = gen.implex(ped, [126], type="IND")
    assert ind_m[62, 0] == 2.0 / 2.0 ** 62 * 100.0
    ind, fa, mo = doubling_chain(64)
    with pytest.raises(ValueError):
        gen.implex(_ped(gen, ind, fa, mo), [127])


@pytest.mark.parametrize("seed", range(3))
def test_against_the_other_sweeps(gen, seed):
    """onlyNewAnc counts are the histogram of gen.meioses' rows and sum to the number of ancestors; the default counts are at most
    the path counts of gen.completeness."""
    rng = np.random.default_rng(500 + seed)
    ind, fa, mo, _ = random_pedigree(rng, 600, p_founder=0.1, p_one_parent=0.1, p_selfing=0.02, max_back=80, max_depth=12)
    ped = _ped(gen, ind, fa, mo)
    pro = rng.choice(ind, size=70, replace=True).astype(np.int64)
    new = gen.ImplexPlan(ind, fa, mo, pro, only_new=True)
    every = gen.ImplexPlan(ind, fa, mo, pro)
    comp = gen.CompletenessPlan(ind, fa, mo, pro)
    try:
        for h in (new, every, comp):
            h.compute()
        G = new.generations
        assert G == every.generations == comp.generations
        dist = gen.meioses(ped, pro, ped.ind)
        hist = np.stack([(dist == g).sum(axis=1) for g in range(G)], axis=1).astype(np.int64)
        _same(new.counts(), hist)
        for i in range(0, len(pro), 9):
            assert int(new.counts()[i, 1:].sum()) == len(gen.ancestor(ped, int(pro[i])))
        assert np.all(every.counts() <= comp.counts()) and np.all(new.counts() <= every.counts())
    finally:
        for h in (new, every, comp):
            h.close()


def test_equal_to_completeness_without_repeated_ancestors(gen):
    """A complete binary ascent of 6 generations: every ancestor is met once, implex and completeness agree."""
    n = 2 ** 7 - 1                                    # heap order from the top: the parents of k are 2k and 2k + 1
    ids = np.arange(1, n + 1, dtype=np.int64)
    fa = np.where(2 * ids + 1 <= n, 2 * ids, 0)
    mo = np.where(2 * ids + 1 <= n, 2 * ids + 1, 0)
    ped = gen.genealogy({"ind": ids, "father": fa, "mother": mo, "sex": np.ones(n, dtype=np.int64)})
    pro = [1, 2, 5]
    imp = gen.ImplexPlan(*_args(ped), pro)
    comp = gen.CompletenessPlan(*_args(ped), pro)
    try:
        imp.compute()
        comp.compute()
        assert imp.counts()[0].tolist() == [1, 2, 4, 8, 16, 32, 64]
        _same(imp.counts(), comp.counts())
        _same(imp.result_to_host(), comp.result_to_host())
    finally:
        imp.close()
        comp.close()
    _same(gen.implex(ped, pro), gen.completeness(ped, pro))
