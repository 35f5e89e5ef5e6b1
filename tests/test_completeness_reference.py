"""gen.completeness (src/describe.jl:73-125) and gen.depth (src/describe.jl:43-66) on the CPU: the two oracles of
tests/completeness_oracle.py against each other, against the reference's pins and against a hand-written matrix; the host-only
parts of the library (planning without a GPU, the number of generations, argument errors, gen.depth, gen.nomen / nowomen / noind,
Pedigree.show(), exports)."""
import ctypes
import os
import re

import numpy as np
import pytest

from completeness_oracle import completeness_exact, completeness_literal, depth_exact, depth_literal, mean_fraction
from test_occ_reference import QUIRK_PRO, doubling_chain, quirk_pedigree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# geneaJi with default arguments (pro = [1, 2, 29]): test/runtests.jl:68-69 pins [8, 1] (1-based) and genNo = [0, 4, 6]
JI_IND = np.array([[100., 100., 100.], [100., 100., 100.], [100., 100., 100.], [100., 100., 75.], [81.25, 81.25, 25.],
                   [50., 50., 12.5], [25., 25., 6.25], [3.125, 3.125, 0.]])
JI_MEAN_0_4_6 = np.array([[100.], [62.5], [18.75]])
# genea140 with default arguments (140 probands): path counts summed per generation, their sum and the largest single count
G140_TOTALS = [140, 280, 560, 1096, 2142, 4076, 7666, 14450, 27394, 51754, 92092, 131784, 125516, 78194, 29974, 7268, 1122, 50]
G140_SUM, G140_MAX = 575_558, 4_474
G140_SHOW = ("A pedigree with:\n41523 individuals;\n68248 parent-child relations;\n20773 men;\n20750 women;\n140 subjects;\n"
             "18 generations.")                                                            # test/runtests.jl:18-20

# tests/test_occ_reference.py: quirk_pedigree with pro = [12, 8, 3, 12, 10, 1]: a leaf, its father (a proband that is a parent of
# another proband), 3, the leaf again, a founder without children, a founder with children; 4 and 9 have one parent.
#   3 = (1, 2): [1, 2];  4 = (1, -): [1, 1];  6 = (3, 5): [1, 2, 2];  7 = (3, 4): [1, 2, 3];  8 = (6, 7): [1, 2, 4, 5];
#   9 = (4, -): [1, 1, 1];  12 = (8, 9): [1, 2, 3, 5, 5]
QUIRK_COUNTS = np.array([[1, 2, 3, 5, 5], [1, 2, 4, 5, 0], [1, 2, 0, 0, 0], [1, 2, 3, 5, 5], [1, 0, 0, 0, 0], [1, 0, 0, 0, 0]], dtype=np.int64)
QUIRK_IND = np.array([[100., 100., 100., 100., 100., 100.],
                      [100., 100., 100., 100., 0., 0.],
                      [75., 100., 0., 75., 0., 0.],
                      [62.5, 62.5, 0., 62.5, 0., 0.],
                      [31.25, 0., 0., 31.25, 0., 0.]])
QUIRK_MEAN = np.array([[100.], [400. / 6], [250. / 6], [187.5 / 6], [62.5 / 6]])


def _args(ped):
    return ped.ind, ped.father, ped.mother


def test_oracles_reproduce_the_geneaJi_pins(gen):
    ped = gen.genealogy(gen.geneaJi)
    pro = gen.pro(ped)
    assert list(pro) == [1, 2, 29]
    counts, exact = completeness_exact(*_args(ped), pro)
    for ind_matrix in (completeness_literal(*_args(ped), pro, type="IND"), exact):
        assert ind_matrix[7, 0] == 3.125
        assert np.array_equal(ind_matrix, JI_IND)
    assert np.array_equal(completeness_literal(*_args(ped), pro, genNo=[0, 4, 6]), JI_MEAN_0_4_6)
    assert [float(mean_fraction(counts)[g]) for g in (0, 4, 6)] == [100.0, 62.5, 18.75]
    assert depth_literal(*_args(ped)) == depth_exact(*_args(ped)) == 8


def test_oracles_reproduce_the_genea140_pins(gen):
    ped = gen.genealogy(gen.genea140)
    pro = gen.pro(ped)
    assert len(pro) == 140
    counts, exact = completeness_exact(*_args(ped), pro)
    assert counts.shape == (140, 18) and counts.dtype == np.int64
    assert [int(v) for v in counts.sum(axis=0)] == G140_TOTALS
    assert int(counts.sum()) == G140_SUM and int(counts.max()) == G140_MAX
    assert np.array_equal(completeness_literal(*_args(ped), pro, type="IND"), exact)
    assert depth_exact(*_args(ped)) == 18 and depth_exact(*_args(ped), leaves_only=True) == 18


def test_quirks_in_both_oracles(gen):
    ped = quirk_pedigree(gen)
    counts, exact = completeness_exact(*_args(ped), QUIRK_PRO)
    assert np.array_equal(counts, QUIRK_COUNTS)
    assert np.array_equal(exact, QUIRK_IND)
    assert np.array_equal(completeness_literal(*_args(ped), QUIRK_PRO, type="IND"), QUIRK_IND)
    assert np.array_equal(completeness_literal(*_args(ped), QUIRK_PRO), QUIRK_MEAN)
    assert np.array_equal(completeness_literal(*_args(ped), QUIRK_PRO, genNo=[4, 0, 4], type="IND"), QUIRK_IND[[4, 0, 4]])
    assert completeness_literal(*_args(ped), QUIRK_PRO, type="SUM") is None
    assert [float(f) for f in mean_fraction(counts)] == [float(v) for v in QUIRK_MEAN[:, 0]]
    with pytest.raises(KeyError):
        completeness_literal(*_args(ped), [8, 99])
    with pytest.raises(KeyError):
        completeness_exact(*_args(ped), [8, 99])
    with pytest.raises(ValueError):
        completeness_literal(*_args(ped), [])
    with pytest.raises(IndexError):
        completeness_literal(*_args(ped), QUIRK_PRO, genNo=[5])
    assert depth_literal(*_args(ped)) == depth_exact(*_args(ped)) == 5
    assert completeness_literal(*_args(ped), [10, 1], type="IND").shape == (1, 2)       # founders only: generation 0


def test_doubling_chain_in_the_exact_oracle():
    ind, fa, mo = doubling_chain(63)
    counts, exact = completeness_exact(ind, fa, mo, [2 * 63, 2 * 63 - 1])
    assert counts.shape == (2, 63) and int(counts[0, 62]) == 2 ** 62
    assert np.array_equal(exact, np.full((63, 2), 100.0))
    assert depth_exact(ind, fa, mo) == 63


def test_plans_are_host_only_and_report_their_generations(gen):
    ped = gen.genealogy(gen.genea140)
    for totals_only in (False, True):
        h = gen.CompletenessPlan(*_args(ped), gen.pro(ped), totals_only=totals_only)
        try:
            st = h.stats()
            assert h.generations == 18 and h.shape == (140, 18)
            assert st["peak_slots"] > 0 and st["sweep_ms"] == 0.0 and st["row_entries"] == 24
        finally:
            h.close()
    ped = quirk_pedigree(gen)
    for pro, G in ((QUIRK_PRO, 5), ([8, 3], 4), ([3, 1], 2), ([10, 1, 10], 1)):
        h = gen.CompletenessPlan(*_args(ped), pro)
        try:
            assert h.generations == G
        finally:
            h.close()


def test_argument_errors_raise_without_gpu(gen):
    ped = quirk_pedigree(gen)
    with pytest.raises(KeyError):
        gen.completeness(ped, [8, 99])
    with pytest.raises(KeyError):
        gen.CompletenessPlan(*_args(ped), [0])
    with pytest.raises(ValueError):
        gen.completeness(ped, type="SUM")
    with pytest.raises(ValueError):
        gen.completeness(ped, [])
    for type_ in ("IND", "MEAN"):
        with pytest.raises(IndexError):
            gen.completeness(ped, QUIRK_PRO, genNo=[0, 5], type=type_)
        with pytest.raises(IndexError):
            gen.completeness(ped, QUIRK_PRO, genNo=[-1], type=type_)


def test_depth_limit_is_62_generations_above_the_probands(gen):
    ind, fa, mo = doubling_chain(64)
    with pytest.raises(ValueError):
        gen.CompletenessPlan(ind, fa, mo, [2 * 64])
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)})
    for type_ in ("IND", "MEAN"):
        with pytest.raises(ValueError):
            gen.completeness(ped, type=type_)
    h = gen.CompletenessPlan(ind, fa, mo, [2 * 63])                   # a proband of generation 63 of the same pedigree
    h.close()
    ind, fa, mo = doubling_chain(63)
    h = gen.CompletenessPlan(ind, fa, mo, [2 * 63])
    try:
        assert h.generations == 63
    finally:
        h.close()
    # one proband: a total is a count and fits; two probands: 62 + 1 bits do not
    gen.CompletenessPlan(ind, fa, mo, [2 * 63], totals_only=True).close()
    with pytest.raises(ValueError):
        gen.CompletenessPlan(ind, fa, mo, [2 * 63, 2 * 63 - 1], totals_only=True)
    gen.CompletenessPlan(ind, fa, mo, [2 * 62, 2 * 62 - 1], totals_only=True).close()


def test_depth_and_counts_of_the_bundled_pedigrees(gen):
    ped = gen.genealogy(gen.genea140)
    assert gen.depth(ped) == 18                                       # test/runtests.jl:32
    assert (gen.nomen(ped), gen.nowomen(ped), gen.noind(ped)) == (20773, 20750, 41523)          # :21-23
    assert ped.show() == G140_SHOW
    assert repr(ped) == "Pedigree(41523 individuals)"
    ji = gen.genealogy(gen.geneaJi)
    assert gen.depth(ji) == depth_literal(*_args(ji)) == 8
    assert ji.show().endswith("3 subjects;\n8 generations.")


def test_depth_and_show_on_small_pedigrees(gen):
    one = gen.genealogy({"ind": [7], "father": [0], "mother": [0], "sex": [1]})
    assert gen.depth(one) == 1 and (gen.nomen(one), gen.nowomen(one), gen.noind(one)) == (1, 0, 1)
    assert one.show() == "A pedigree with:\n1 individual;\n0 parent-child relations;\n1 man;\n0 women;\n1 subject;\n1 generation."
    trio = gen.genealogy({"ind": [1, 2, 3], "father": [0, 0, 1], "mother": [0, 0, 0], "sex": [1, 2, 2]})
    assert trio.show() == "A pedigree with:\n3 individuals;\n1 parent-child relation;\n1 man;\n2 women;\n2 subjects;\n2 generations."
    empty = gen.genealogy({"ind": [], "father": [], "mother": [], "sex": []})
    assert gen.depth(empty) == 0 and gen.noind(empty) == 0
    founders = gen.genealogy({"ind": [3, 1, 2], "father": [0, 0, 0], "mother": [0, 0, 0], "sex": [1, 2, 0]})
    assert gen.depth(founders) == 1 and (gen.nomen(founders), gen.nowomen(founders)) == (1, 1)
    assert "1 man;\n2 women;\n3 subjects;\n1 generation." in founders.show()      # show counts whoever is not a man as a woman
    ped = quirk_pedigree(gen)
    assert gen.depth(ped) == depth_literal(*_args(ped)) == 5
    # (the deepest individual never has a child, so the subjects' depth that show prints is the depth of the pedigree)
    from genlib_jl_amd import _capi
    ind, fa, mo = np.array([5, 4, 3, 2, 1]), np.array([4, 0, 2, 1, 0]), np.zeros(5, dtype=np.int64)      # no order is assumed
    assert _capi.genealogy_depth(ind, fa, mo) == _capi.genealogy_depth(ind, fa, mo, leaves_only=True) == 3
    assert depth_exact(ind, fa, mo, leaves_only=True) == depth_literal(ind, fa, mo) == 3
    with pytest.raises(KeyError):
        _capi.genealogy_depth([1, 2], [0, 9], [0, 0])
    with pytest.raises(ValueError):
        _capi.genealogy_depth([1, 2], [2, 1], [0, 0])                 # a cycle


def test_depth_matches_the_oracles_on_a_synthetic_pedigree(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(3000, 300, 9, skip_permille=50)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    assert gen.depth(ped) == depth_exact(ind, fa, mo) == depth_literal(ind, fa, mo)
    h = gen.CompletenessPlan(*_args(ped), gen.pro(ped))
    try:
        assert h.generations == depth_exact(ind, fa, mo, leaves_only=True)
    finally:
        h.close()


def test_symbols_are_exported_and_called_by_the_julia_shim(gen):
    from genlib_jl_amd import _capi
    src = open(os.path.join(ROOT, "genlib.jl_amd", "julia", "GenLibAMD.jl")).read()
    called = set(re.findall(r"\(:(genphi_(?:comp_[a-z_]+|genealogy_depth)), libgenphi\)", src))
    assert called == {"genphi_comp_create", "genphi_comp_compute", "genphi_comp_generations", "genphi_comp_result_to_host",
                      "genphi_comp_totals", "genphi_comp_destroy", "genphi_genealogy_depth"}
    header = open(os.path.join(ROOT, "include", "genphi.h")).read()
    assert "#define GENPHI_COMP_MAX_GENERATIONS 62" in header
    L = ctypes.CDLL(_capi.LIB_PATH)
    for name in called | {"genphi_comp_result_device", "genphi_comp_counts_to_host", "genphi_comp_stats"}:
        assert hasattr(L, name) and name in _capi.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, header), name
