"""The MRCA family (src/identify.jl:83-199, src/describe.jl:241-300) on the CPU: the two oracles of tests/mrca_oracle.py against
each other, against the reference's pins on geneaJi and against hand-written matrices; the host-only parts of the library
(gen.ancestor, the MRCA filter, planning gen.meioses without a GPU, the depth limit, exports)."""
import ctypes
import os
import re

import numpy as np
import pytest

import mrca_oracle as MO
from test_occ_reference import QUIRK_ANC, QUIRK_PRO, doubling_chain, quirk_pedigree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# test/runtests.jl:43-46, 62, 64, 67 (geneaJi)
JI_IDS = [1, 2, 29]
JI_MRCA = np.array([14, 20], dtype=np.int64)
JI_MEIOSES = np.array([[4, 4], [4, 4], [3, 3]], dtype=np.int64)
JI_FOUNDERS = np.array([17, 19, 20, 25, 26], dtype=np.int64)
# genea140: (number of first probands, common ancestors, MRCAs); the largest entry of the first matrix
G140_SETS = [(2, 354, 108), (10, 106, 42), (140, 0, 0)]
G140_MAX2 = 14

# shortest ascents on quirk_pedigree (tests/test_occ_reference.py) for QUIRK_PRO x QUIRK_ANC = [12, 8, 3, 12, 10, 1] x
# [1, 1, 3, 8, 10, 5, 11, 4]: 12 reaches 1 in 3 steps through 9 and 4, not in 4 steps through the requested ancestor 3; 8, 10 and 1 are
# probands at distance 0 from themselves; 11 is unrelated; 4 has one parent
QUIRK_MEIOSES = np.array([
    [3, 3, 3, 1, -1, 3, -1, 2],
    [3, 3, 2, 0, -1, 2, -1, 2],
    [1, 1, 0, -1, -1, -1, -1, -1],
    [3, 3, 3, 1, -1, 3, -1, 2],
    [-1, -1, -1, -1, 0, -1, -1, -1],
    [0, 0, -1, -1, -1, -1, -1, -1],
], dtype=np.int16)


def shortcut_pedigree():
    """1 founder; 2 = (1, -); 3 = (2, -); 4 = (3, 1): 4 reaches 1 in one step past the requested ancestors 3 and 2; 5 = (4, -)."""
    return np.arange(1, 6), np.array([0, 1, 2, 3, 4]), np.array([0, 0, 0, 1, 0])


SHORTCUT_PRO, SHORTCUT_ANC = [5, 4, 3], [1, 2, 3, 4]
SHORTCUT_MEIOSES = np.array([[2, 3, 2, 1], [1, 2, 1, 0], [2, 1, 0, -1]], dtype=np.int16)


def _args(ped):
    return ped.ind, ped.father, ped.mother


def test_oracles_reproduce_the_geneaJi_pins(gen):
    ped = gen.genealogy(gen.geneaJi)
    for find in (MO.find_mrca_literal, MO.find_mrca_exact):
        anc, M, _ = find(*_args(ped), JI_IDS)
        assert np.array_equal(anc, JI_MRCA) and np.array_equal(M, JI_MEIOSES)
    for find in (MO.find_founders_literal, MO.find_founders_exact):
        assert np.array_equal(find(*_args(ped), JI_IDS), JI_FOUNDERS)
    assert MO.find_distance_literal(*_args(ped), [1, 2], 25) == 12
    assert int(MO.meioses_exact(*_args(ped), [1, 2], [25]).sum()) == 12
    assert MO.min_distance_mrca_literal(*_args(ped), [2, 29]) == 7
    anc, M, _ = MO.find_mrca_exact(*_args(ped), [2, 29])
    assert int((M[0] + M[1]).min()) == 7


def test_oracles_agree_on_genea140_and_hold_its_pins(gen):
    ped = gen.genealogy(gen.genea140)
    pro = gen.pro(ped)
    assert [int(p) for p in pro[:2]] == [217891, 218089]
    for n, n_common, n_mrca in G140_SETS:
        ea, eM, ec = MO.find_mrca_exact(*_args(ped), pro[:n])
        assert (ec, len(ea)) == (n_common, n_mrca)
        if n <= 10:
            la, lM, lc = MO.find_mrca_literal(*_args(ped), pro[:n])
            assert lc == ec and np.array_equal(la, ea) and np.array_equal(lM, eM)
        if n == 2:
            assert int(eM.max()) == G140_MAX2
    # all 140 probands against every individual that has a child: both oracles, every pair
    anc = np.setdiff1d(ped.ind, pro)[::7]
    assert np.array_equal(MO.meioses_literal(*_args(ped), pro, anc), MO.meioses_exact(*_args(ped), pro, anc))
    assert np.array_equal(MO.find_founders_literal(*_args(ped), pro[:10]), MO.find_founders_exact(*_args(ped), pro[:10]))


def test_hand_built_matrices_in_both_oracles(gen):
    ped = quirk_pedigree(gen)
    for fn in (MO.meioses_literal, MO.meioses_exact):
        assert np.array_equal(fn(*_args(ped), QUIRK_PRO, QUIRK_ANC), QUIRK_MEIOSES)
        assert np.array_equal(fn(*shortcut_pedigree(), SHORTCUT_PRO, SHORTCUT_ANC), SHORTCUT_MEIOSES)
        assert fn(*_args(ped), [], [1, 2]).shape == (0, 2) and fn(*_args(ped), [8, 9], []).shape == (2, 0)
        with pytest.raises(KeyError):
            fn(*_args(ped), [8, 99], [1])
        with pytest.raises(KeyError):
            fn(*_args(ped), [8], [99])
    # 12 and 7: common ancestors 1, 2, 3, 4; 3 and 4 have no common child
    for find in (MO.find_mrca_literal, MO.find_mrca_exact):
        anc, M, n_common = find(*_args(ped), [12, 7, 12])
        assert anc.tolist() == [3, 4] and n_common == 4 and M.tolist() == [[3, 2], [1, 1], [3, 2]]


def test_ancestor_matches_the_oracle(gen):
    ped = gen.genealogy(gen.genea140)
    par = MO._parents(*_args(ped))
    pro = gen.pro(ped)
    for ids in (int(pro[0]), [int(pro[3])], pro[:7], [int(gen.founder(ped)[0])], []):
        got = gen.ancestor(ped, ids)
        assert got.dtype == np.int64 and got.tolist() == MO.ancestor_literal(par, ids if isinstance(ids, int) else list(ids))
    assert len(gen.ancestor(ped, int(pro[0]))) <= 6218 and max(len(gen.ancestor(ped, int(p))) for p in pro) == 6218
    ji = gen.genealogy(gen.geneaJi)
    assert 1 not in gen.ancestor(ji, [1, 2]).tolist()              # strict
    with pytest.raises(KeyError):
        gen.ancestor(ped, [int(pro[0]), 10 ** 9])
    with pytest.raises(KeyError):
        gen.ancestor(ped, 10 ** 9)


def test_mrca_filter_equals_setdiff(gen):
    """No common child <=> not an ancestor of another common ancestor, on the common sets of genea140 and of a synthetic pedigree
    with one-parent members."""
    from genlib_jl_amd import _capi, synth
    ped = gen.genealogy(gen.genea140)
    pro = gen.pro(ped)
    cases = [(ped, pro[:2], 354, 108), (ped, pro[:10], 106, 42), (ped, pro[[5, 77]], None, None), (ped, pro, 0, 0)]
    ind, fa, mo, sex, spro = synth.random_mating(4000, 400, 10, skip_permille=50)
    mo = mo.copy()
    mo[(np.arange(len(ind)) % 13 == 5) & (fa != 0)] = 0
    sped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    cases += [(sped, spro[:2], None, None), (sped, spro[[3, 9, 200]], None, None)]
    for p, ids, n_common, n_mrca in cases:
        par = MO._parents(*_args(p))
        mrcas, common = MO.mrca_ids_literal(par, ids)
        if n_common is not None:
            assert (len(common), len(mrcas)) == (n_common, n_mrca)
        got = _capi.mrca_filter(*_args(p), np.array(common, dtype=np.int64))
        assert got.tolist() == mrcas
    assert _capi.mrca_filter(*_args(ped), np.zeros(0, dtype=np.int64)).shape == (0,)
    with pytest.raises(KeyError):
        _capi.mrca_filter(*_args(ped), np.array([10 ** 9]))


def test_dist_plans_are_host_only(gen):
    """create plans on the host: errors, empty lists and the depth limit need no GPU; an empty result needs none to compute."""
    ped = quirk_pedigree(gen)
    with pytest.raises(KeyError):
        gen.DistPlan(*_args(ped), [8, 99], [1])
    with pytest.raises(KeyError):
        gen.DistPlan(*_args(ped), [8], [1, 99])
    with pytest.raises(KeyError):
        gen.meioses(ped, pro=[0])
    h = gen.DistPlan(*_args(ped), QUIRK_PRO, QUIRK_ANC)
    try:
        st = h.stats()
        assert st["peak_slots"] > 0 and st["sweep_ms"] == 0.0 and st["row_bits"] == 16
    finally:
        h.close()
    for pro, anc in (([], [1, 2]), ([8, 9], []), ([], [])):
        out = gen.meioses(ped, pro=pro, ancestors=anc)
        assert out.shape == (len(pro), len(anc)) and out.dtype == np.int16
    # a signed 16-bit distance covers 32,767 steps: a chain of 32,768 generations plans, one more is refused
    from genlib_jl_amd import _capi
    assert _capi.GENPHI_DIST_MAX_STEPS == 32767
    ind, fa, mo = doubling_chain(32768)
    gen.DistPlan(ind, fa, mo, [2 * 32768], [1]).close()
    ind, fa, mo = doubling_chain(32769)
    with pytest.raises(ValueError, match="32767"):
        gen.DistPlan(ind, fa, mo, [2 * 32769], [1])
    assert "GENPHI_DIST_MAX_STEPS 32767" in open(os.path.join(ROOT, "include", "genphi.h")).read()


def test_argument_errors_without_gpu(gen):
    ped = gen.genealogy(gen.geneaJi)
    for call in (lambda: gen.findMRCA(ped, [1, 999]), lambda: gen.findMRCA(ped, [999]), lambda: gen.findFounders(ped, [999, 1]),
                 lambda: gen.findDistance(ped, [1, 999], 25), lambda: gen.findDistance(ped, [1, 2], 999),
                 lambda: gen._findMinDistanceMRCA(ped, [999, 2])):
        with pytest.raises(KeyError):
            call()
    for call in (lambda: gen.findDistance(ped, [1], 25), lambda: gen.findDistance(ped, [], 25), lambda: gen._findMinDistanceMRCA(ped, [2])):
        with pytest.raises(IndexError):
            call()
    # founders have no ancestors: no candidates, nothing for the GPU to do
    m = gen.findMRCA(ped, [17, 19])
    assert m.individuals.tolist() == [17, 19] and m.ancestors.shape == (0,) and m.meioses.shape == (2, 0) and m.meioses.dtype == np.int64
    assert gen.findFounders(ped, [17]).shape == (0,)
    assert "GenMatrix(individuals=[17, 19], ancestors=[], meioses=[[], []])" == repr(m)


def test_symbols_are_exported_and_called_by_the_julia_shim(gen):
    from genlib_jl_amd import _capi
    src = open(os.path.join(ROOT, "genlib.jl_amd", "julia", "GenLibAMD.jl")).read()
    called = set(re.findall(r"\(:(genphi_(?:dist_[a-z_]+|ancestors|mrca_filter)), libgenphi\)", src))
    assert called == {"genphi_dist_create", "genphi_dist_compute", "genphi_dist_result_to_host", "genphi_dist_destroy",
                      "genphi_ancestors", "genphi_mrca_filter"}
    L = ctypes.CDLL(_capi.LIB_PATH)
    for name in called | {"genphi_dist_result_device", "genphi_dist_stats"}:
        assert hasattr(L, name) and name in _capi.EXPORTED_SYMBOLS, name
