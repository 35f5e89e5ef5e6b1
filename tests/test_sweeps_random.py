"""The five ancestor sweeps (gen.gc, gen.occ, gen.rec, gen.meioses, gen.completeness) at the places where their kernels change form, and a
short fixed-seed round of tests/stress_sweeps.py.  Every comparison is with the Python oracles of tests/*_oracle.py and exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

import stress_sweeps as S
from completeness_oracle import completeness_exact
from gc_oracle import gc_exact_rows, gc_literal
from mrca_oracle import meioses_exact
from occ_oracle import occ_exact, rec_exact
from test_gc_gpu import _mixed_lists, _one_parent_synth
from test_occ_reference import doubling_chain

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ALL_FORMS = {1, 2, 4, 8, 16, 32, 64}


def _ped(gen, ind, fa, mo, sex=None):
    sex = np.ones(len(ind), dtype=np.int64) if sex is None else sex
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})


def _args(ped):
    return ped.ind, ped.father, ped.mother


def _same(got, want, bits=False):
    d = S._differs(got, want, bits)
    assert d is None, d


def test_sweep_stress_short():
    """120 fixed-seed cases of tests/stress_sweeps.py: random pedigrees (random mating with skipped generations, arbitrary pedigrees with
    founders anywhere, one-parent members and selfing, inbred pedigrees of 33 - 52 generations) x mixed proband and ancestor lists x forced
    panel widths and panels per launch x occ's row width, every family against its oracle, every handle computed twice.  No case is
    skipped.  The oracles take about 12 s of CPU for the 120 cases; measured on an MI355X machine the whole round takes 4.3 - 4.8 s (two runs)."""
    out = subprocess.run([sys.executable, os.path.join(HERE, "stress_sweeps.py"), "120", "20261017"], cwd=HERE, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    last = out.stdout.splitlines()[-1]
    assert last.startswith("sweep stress: 120 cases, 0 failures"), out.stdout[-3000:]
    assert ", 0 failures" in last


@pytest.fixture(scope="module")
def mixed(gen):
    """Overlapping generations and one-parent members; 52 probands (leaves, non-leaves, founders, repeats) x 300 ancestors (founders,
    non-founders, repeats, probands, an unrelated founder): ragged against every forced width below."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, _ = _one_parent_synth(synth)
    ped = _ped(gen, ind, fa, mo, sex)
    pro, anc = _mixed_lists(ped, gen, np.random.default_rng(300), 300)
    return ped, pro, anc


# forced panel widths: the upper end of every lanes-per-row class of the family, odd widths, widths that are no multiple of 8
GC_WIDTHS = [1, 2, 3, 4, 7, 8, 13, 16, 32, 33, 64, 128, 131]
OCC32_WIDTHS = [3, 4, 8, 11, 16, 32, 64, 65, 128, 140]
OCC64_WIDTHS = [1, 2, 4, 7, 8, 16, 32, 64, 128, 131]
DIST_WIDTHS = [3, 8, 16, 20, 32, 64, 65, 128, 130, 256, 257]       # 3, 20, 65, 130, 257: panels start off a multiple of 8 columns
REC_WIDTHS = [100, 128, 200, 400, 800, 1600, 3200, 7399]           # bit rows: 128 columns per 16-byte vector
COMP_GENERATIONS = [1, 2, 3, 5, 9, 17, 33, 60]


def test_every_kernel_form_is_reached(gen, mixed, monkeypatch):
    """Every lanes-per-row instantiation (1, 2, 4, 8, 16, 32, 64) of the step kernels of every family, selected by a forced panel width
    (completeness: by the number of generations) and checked against the oracle.  The widths imply all seven forms by the rule of each
    file (restated in tests/stress_sweeps.py), and the handle reports the forced width."""
    ped, pro, anc = mixed
    args = _args(ped)
    assert {S.gc_lanes(w) for w in GC_WIDTHS} == ALL_FORMS
    assert {S.occ_lanes(w, 32) for w in OCC32_WIDTHS} == ALL_FORMS and {S.occ_lanes(w, 64) for w in OCC64_WIDTHS} == ALL_FORMS
    assert {S.dist_lanes(w) for w in DIST_WIDTHS} == ALL_FORMS and {S.rec_lanes(w) for w in REC_WIDTHS} == ALL_FORMS
    assert {S.lanes_per_row(g) for g in COMP_GENERATIONS} == ALL_FORMS
    assert max(GC_WIDTHS + OCC32_WIDTHS + OCC64_WIDTHS + DIST_WIDTHS) < len(anc)

    want_gc = gc_exact_rows(*args, pro, anc)
    _same(want_gc, gc_literal(*args, pro, anc), bits=True)              # (10 generations: the two oracles agree)
    for w in GC_WIDTHS:
        monkeypatch.setenv("GENPHI_GC_PANEL", str(w))
        h = gen.GCPlan(*args, pro, anc)
        try:
            h.compute()
            assert h.stats()["panel_cols"] == w
            _same(h.result_to_host(), want_gc, bits=True)
        finally:
            h.close()

    want_occ = occ_exact(*args, pro, anc)
    want_rec = rec_exact(*args, pro, anc)
    for rows64, widths in ((False, OCC32_WIDTHS), (True, OCC64_WIDTHS)):
        for w in widths:
            monkeypatch.setenv("GENPHI_OCC_PANEL", str(w))
            h = gen.OccPlan(*args, pro, anc, rows64=rows64)
            t = gen.OccPlan(*args, pro, anc, total_only=True, rows64=rows64)
            r = gen.RecPlan(*args, pro, anc)
            try:
                for x in (h, t, r):
                    x.compute()
                    assert x.stats()["panel_cols"] == w
                assert h.stats()["row_bits"] == t.stats()["row_bits"] == (64 if rows64 else 32)
                _same(h.result_to_host().T, want_occ)
                _same(t.totals(), want_occ.sum(axis=1, dtype=np.int64))
                _same(r.result(), want_rec)
            finally:
                h.close()
                t.close()
                r.close()

    want_dist = meioses_exact(*args, pro, anc)
    for w in DIST_WIDTHS:
        monkeypatch.setenv("GENPHI_DIST_PANEL", str(w))
        h = gen.DistPlan(*args, pro, anc)
        try:
            h.compute()
            assert h.stats()["panel_cols"] == w
            _same(h.result_to_host(), want_dist)
        finally:
            h.close()

    # rec's vectors hold 128 columns: its wide forms need thousands of columns (genea140: 7,399 founders)
    g140 = gen.genealogy(gen.genea140)
    pro140, anc140 = gen.pro(g140), gen.founder(g140)
    assert len(anc140) == 7399
    want_rec = rec_exact(*_args(g140), pro140, anc140)
    for w in REC_WIDTHS:
        monkeypatch.setenv("GENPHI_OCC_PANEL", str(w))
        r = gen.RecPlan(*_args(g140), pro140, anc140)
        try:
            r.compute()
            assert r.stats()["panel_cols"] == w
            _same(r.result(), want_rec)
        finally:
            r.close()

    # completeness: a lane per generation.  Chains of G generations; the probands: the last two members, one of their parents (it waits
    # in its slot: a copy item), a repeat
    for G in COMP_GENERATIONS:
        cped = _ped(gen, *doubling_chain(G))
        cpro = np.array([2 * G, 2 * G - 1, max(2 * G - 3, 1), 2 * G], dtype=np.int64)
        counts, matrix = completeness_exact(*_args(cped), cpro)
        assert counts.shape == (4, G)
        for totals_only in (False, True):
            h = gen.CompletenessPlan(*_args(cped), cpro, totals_only=totals_only)
            try:
                assert h.generations == G
                h.compute()
                assert h.stats()["row_entries"] == (G + 7) // 8 * 8
                _same(h.totals(), counts.sum(axis=0, dtype=np.int64))
                if not totals_only:
                    _same(h.counts(), counts)
                    _same(h.result_to_host().T, matrix)
            finally:
                h.close()


@pytest.mark.parametrize("panel", [None, 16])
@pytest.mark.parametrize("n_items", [1, 63, 64, 65, 128, 129, 257, 769])
def test_total_reductions_at_their_row_group_edges(gen, mixed, monkeypatch, n_items, panel):
    """occ TOTAL and completeness totals_only add 64 items of the last list per row group, four row groups (of 64 lanes) per block: a last
    list of exactly 1, 63, 64, 65, 128, 129 and 4 * 64 * k + 1 (k = 1, 3) items.  Every founder is an ancestor, so every proband has a row
    and the last list holds one item per listed proband: leaves, repeated up to the count.  panel = 16 columns: 16 row groups per wave."""
    ped, _, _ = mixed
    args = _args(ped)
    anc = gen.founder(ped)
    leaves = np.setdiff1d(gen.pro(ped), anc)                                 # with parents: several founders each
    pro = np.resize(leaves[:100], n_items).astype(np.int64)                  # n_items > 100: every leaf listed several times
    assert len(pro) == n_items and not np.isin(pro, np.union1d(ped.father, ped.mother)).any()        # no proband waits in a slot: all in the last list
    if panel is None:
        monkeypatch.delenv("GENPHI_OCC_PANEL", raising=False)
    else:
        monkeypatch.setenv("GENPHI_OCC_PANEL", str(panel))
    want = occ_exact(*args, pro, anc).sum(axis=1, dtype=np.int64)
    assert int(want.sum()) > n_items
    for rows64 in (False, True):
        t = gen.OccPlan(*args, pro, anc, total_only=True, rows64=rows64)
        try:
            t.compute()
            if panel is not None:
                assert t.stats()["panel_cols"] == panel
            _same(t.totals(), want)
            t.compute()                                                       # again on the same handle: the totals start from zero
            _same(t.totals(), want)
        finally:
            t.close()
    counts, _ = completeness_exact(*args, pro)
    c = gen.CompletenessPlan(*args, pro, totals_only=True)
    try:
        c.compute()
        _same(c.totals(), counts.sum(axis=0, dtype=np.int64))
        c.compute()
        _same(c.totals(), counts.sum(axis=0, dtype=np.int64))
    finally:
        c.close()


@pytest.fixture(scope="module")
def genea140_gc(gen):
    ped = gen.genealogy(gen.genea140)
    pro, anc = gen.pro(ped), gen.founder(ped)
    return ped, pro, anc, gc_literal(*_args(ped), pro, anc)


@pytest.mark.parametrize("group", [1, 7, 0])
def test_gc_panels_per_launch(gen, genea140_gc, monkeypatch, group):
    """genea140 in panels of 100 columns (74 panels, the last one of 99), one, seven (the last launch holds four) and as many per launch
    as the memory holds (0: no hook)."""
    monkeypatch.setenv("GENPHI_GC_PANEL", "100")
    if group:
        monkeypatch.setenv("GENPHI_GC_PANELS_PER_LAUNCH", str(group))
    else:
        monkeypatch.delenv("GENPHI_GC_PANELS_PER_LAUNCH", raising=False)
    ped, pro, anc, want = genea140_gc
    h = gen.GCPlan(*_args(ped), pro, anc)
    try:
        h.compute()
        assert h.stats()["panel_cols"] == 100
        out = h.result_to_host()
    finally:
        h.close()
    _same(out, want, bits=True)
    assert float(np.sum(out, dtype=np.float64)) == 140.0
