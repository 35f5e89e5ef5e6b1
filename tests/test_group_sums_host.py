"""Host side of gen.phiMeanGroups (no GPU): the population file, the oracle of tests/group_sums_oracle.py on a case computed by
hand, the proband order and labels the function plans with, the exported symbol and its binding."""
import ctypes
import os
import re

import numpy as np
import pytest

import group_sums_oracle as GO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POP140 = os.path.join(ROOT, "tests", "golden", "pop140.csv")
SIZES = {"Gaspesia-Acadian": 20, "Gaspesia-FrenchCanadian": 20, "Gaspesia-Loyalist": 20, "Montreal": 22, "NorthShore": 20,
         "Quebec": 16, "Saguenay": 22}


def test_pop_reads_the_reference_population_file(gen):
    pop = gen._pop(POP140)
    assert len(pop) == 140 and pop[217891] == "Saguenay"                    # test/runtests.jl:90-94
    names, counts = np.unique(list(pop.values()), return_counts=True)
    assert dict(zip(names.tolist(), counts.tolist())) == SIZES
    ped = gen.genealogy(gen.genea140)
    assert set(pop) == set(gen.pro(ped).tolist())                           # the 140 childless members of genea140


def test_oracle_on_a_case_computed_by_hand():
    phi = np.array([[.5, .25, .125, 0], [.25, .5, 0, .125], [.125, 0, .5, .0625], [0, .125, .0625, .5]], dtype=np.float32)
    sums, diag, rows, cols = GO.group_sums(phi, [0, 1, 0, -1], 3)
    assert sums.tolist() == [[1.25, .25, 0], [.25, .5, 0], [0, 0, 0]]
    assert diag.tolist() == [1.0, .5, 0] and rows.tolist() == [2, 1, 0] and cols.tolist() == [2, 1, 0]
    sums, diag, rows, cols = GO.group_sums(phi[2:], [0, 1, 0, -1], 2, row_begin=2)      # a shard: rows 2 and 3
    assert sums.tolist() == [[.625, 0], [0, 0]] and diag.tolist() == [.5, 0] and rows.tolist() == [1, 0] and cols.tolist() == [2, 1]
    mean, bound = GO.mean_table(GO.group_sums(phi, [0, 1, 0, -1], 3))
    assert mean[0, 0] == .125 and mean[0, 1] == .125 and np.isnan(mean[1, 1]) and np.isnan(mean[2, 0]) and np.all(bound[:2, :1] < 1e-15)
    assert GO.gamma(1) == 0 and GO.gamma(3) == 2 * GO.U / (1 - 2 * GO.U)


def test_mean_from_group_sums_matches_the_oracle_table(gen):
    phi = np.array([[.5, .25, .125, 0], [.25, .5, 0, .125], [.125, 0, .5, .0625], [0, .125, .0625, .5]], dtype=np.float32)
    ref = GO.group_sums(phi, [0, 1, 0, -1], 3)
    got = gen._capi.mean_from_group_sums(ref[0], ref[1], ref[3])
    assert np.array_equal(got, GO.mean_table(ref)[0], equal_nan=True)


def test_group_order_sorts_by_group_name_then_id(gen):
    groups = {30: "b", 10: "b", 20: "a", 40: "c", 5: "a"}
    names, ids, labels = gen._group_order(groups)
    assert names == ["a", "b", "c"] and ids.tolist() == [5, 20, 10, 30, 40] and labels.tolist() == [0, 0, 1, 1, 2]
    assert ids.dtype == np.int64 and labels.dtype == np.int32
    # probands outside groups come last with label -1; a repeated ID counts once; groups without a proband keep their name
    names, ids, labels = gen._group_order(groups, [40, 7, 10, 10, 3, 5])
    assert names == ["a", "b", "c"] and ids.tolist() == [5, 10, 40, 3, 7] and labels.tolist() == [0, 1, 2, -1, -1]
    with pytest.raises(ValueError):
        gen._group_order({})


def test_group_order_of_pop140_is_seven_runs(gen):
    names, ids, labels = gen._group_order(gen._pop(POP140))
    assert names == sorted(SIZES) and np.bincount(labels).tolist() == [SIZES[n] for n in names]
    assert np.all(np.diff(labels) >= 0) and sorted(ids.tolist()) == sorted(gen._pop(POP140))
    for g in range(7):
        assert np.all(np.diff(ids[labels == g]) > 0)


def test_unknown_id_and_empty_groups_raise_before_any_device_work(gen):
    ped = gen.genealogy(gen.geneaJi)
    with pytest.raises(KeyError):
        gen.phiMeanGroups(ped, {1: "x", 12345: "x"})
    with pytest.raises(ValueError):
        gen.phiMeanGroups(ped, {})


def test_symbol_is_exported_declared_and_bound(gen):
    from genlib_jl_amd import _capi
    assert "genphi_result_group_sums" in _capi.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), "genphi_result_group_sums")
    header = open(os.path.join(ROOT, "include", "genphi.h")).read()
    assert re.search(r"\bgenphi_result_group_sums\s*\(", header)
    assert "#define GENPHI_GROUP_SUMS_MAX_GROUPS %d" % _capi.GENPHI_GROUP_SUMS_MAX_GROUPS in header
    assert _capi.GENPHI_GROUP_SUMS_MAX_GROUPS >= 4096
    assert len(_capi.lib().genphi_result_group_sums.argtypes) == 8


def test_argument_errors_need_no_device(gen):
    """Labels and n_groups are checked before the library looks for a resident result."""
    ped = gen.genealogy(gen.geneaJi)
    pl = gen.plan(ped)
    try:
        for labels, g in (([0, 0, 2], 2), ([0, -2, 0], 1), ([0, 0, 0], 0), ([0, 0, 0], gen._capi.GENPHI_GROUP_SUMS_MAX_GROUPS + 1)):
            with pytest.raises(ValueError):
                pl.group_sums(labels, g)
            lab = np.array(labels, dtype=np.int32)
            rc = gen._capi.lib().genphi_result_group_sums(pl._h, g, lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None, None, None, None, None)
            assert rc == gen._capi.GENPHI_ERR_ARG and "genphi_result_group_sums" in gen._capi.last_error()
        with pytest.raises(ValueError):
            pl.group_sums([0, 0], 1)                                        # one label per proband
        with pytest.raises(gen.GenphiDeviceError):
            pl.group_sums([0, 0, 0], 1)                                     # valid arguments, nothing computed
    finally:
        pl.close()
