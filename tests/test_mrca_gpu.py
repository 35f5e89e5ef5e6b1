"""gen.meioses and the MRCA family on the GPU (csrc/dist.hip, csrc/loader.cpp) against the oracles of tests/mrca_oracle.py and the
reference's pins.  Every comparison is exact (np.array_equal)."""
import ctypes

import numpy as np
import pytest

import mrca_oracle as MO
from test_gc_gpu import _mixed_lists, _one_parent_synth
from test_mrca_reference import (G140_MAX2, G140_SETS, JI_FOUNDERS, JI_IDS, JI_MEIOSES, JI_MRCA, QUIRK_MEIOSES, SHORTCUT_ANC,
                                 SHORTCUT_MEIOSES, SHORTCUT_PRO, shortcut_pedigree)
from test_occ_reference import QUIRK_ANC, QUIRK_PRO, doubling_chain, quirk_pedigree

pytestmark = pytest.mark.gpu


def _ped(gen, ind, fa, mo, sex=None, sort=True):
    sex = np.ones(len(ind), dtype=np.int64) if sex is None else sex
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}, sort=sort)


def _args(ped):
    return ped.ind, ped.father, ped.mother


def _same(a, b, dtype=np.int16):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == dtype and a.shape == b.shape, (a.dtype, a.shape, b.shape)
    bad = np.argwhere(a != b)
    assert len(bad) == 0, f"{len(bad)} entries differ, first at {tuple(bad[0])}: {a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}"


def _same_matrix(m, ids, ref):
    """A GenMatrix against the oracle's (ancestors, meioses, ...)."""
    _same(m.individuals, np.asarray(ids, dtype=np.int64), np.int64)
    _same(m.ancestors, ref[0], np.int64)
    _same(m.meioses, ref[1], np.int64)


@pytest.fixture(scope="module")
def genea140(gen):
    ped = gen.genealogy(gen.genea140)
    return ped, gen.pro(ped), gen.founder(ped)


@pytest.fixture(scope="module")
def genea140_exact(genea140):
    ped, pro, anc = genea140
    return MO.meioses_exact(*_args(ped), pro, anc)


@pytest.fixture(scope="module")
def cfg3(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(100_000, 10_000, 20)
    return _ped(gen, ind, fa, mo, sex), pro


def test_geneaJi_pins_through_every_function(gen):
    ped = gen.genealogy(gen.geneaJi)
    m = gen.findMRCA(ped, JI_IDS)                                    # test/runtests.jl:43-46
    _same_matrix(m, JI_IDS, (JI_MRCA, JI_MEIOSES))
    _same(gen.findFounders(ped, JI_IDS), JI_FOUNDERS, np.int64)      # :62
    assert gen.findDistance(ped, [1, 2], 25) == 12                   # :64
    assert gen._findMinDistanceMRCA(ped, [2, 29]) == 7               # :67
    _same(gen.meioses(ped, JI_IDS, JI_MRCA), JI_MEIOSES.astype(np.int16))
    _same(gen.meioses(ped), MO.meioses_literal(*_args(ped), gen.pro(ped), gen.founder(ped)))
    _same_matrix(gen.findMRCA(ped, [29, 1, 29]), [29, 1, 29], MO.find_mrca_literal(*_args(ped), [29, 1, 29]))
    assert gen.findDistance(ped, [14, 1], 14) == 4                   # an ID equal to the ancestor is at distance 0
    assert repr(gen.findMRCA(ped, [1, 2])).startswith("GenMatrix(individuals=[1, 2], ancestors=[")


@pytest.mark.parametrize("n,n_common,n_mrca", G140_SETS)
def test_genea140_findMRCA(gen, genea140, n, n_common, n_mrca):
    ped, pro, _ = genea140
    ref = MO.find_mrca_exact(*_args(ped), pro[:n])
    assert (ref[2], len(ref[0])) == (n_common, n_mrca)
    m = gen.findMRCA(ped, pro[:n])
    _same_matrix(m, pro[:n], ref)
    assert m.meioses.shape == (n, n_mrca)
    if n == 2:
        assert int(m.meioses.max()) == G140_MAX2
        assert gen._findMinDistanceMRCA(ped, pro[:n]) == int((ref[1][0] + ref[1][1]).min())
    _same(gen.findFounders(ped, pro[:n]), MO.find_founders_exact(*_args(ped), pro[:n]), np.int64)


def test_genea140_default_arguments(gen, genea140, genea140_exact):
    ped, pro, anc = genea140
    out = gen.meioses(ped)
    assert out.shape == (140, 7399)
    _same(out, genea140_exact)
    assert int(out.max()) == int(genea140_exact.max()) and int((out >= 0).sum()) == 90_814      # gen.rec's pin: related pairs
    h = gen.DistPlan(*_args(ped), pro, anc)
    try:
        h.compute()
        st = h.stats()
        assert st["row_bits"] == 16 and st["sweep_ms"] > 0 and st["algorithmic_bytes"] > 140 * 7399 * 2
        # the default panel: all columns, or a multiple of 8 columns whose slot rows stay within 150 MiB
        C = st["panel_cols"]
        assert C == 7399 or (C % 8 == 0 and 64 <= C < 7399 and 2 * C * st["peak_slots"] <= 150 << 20)
        ptr, ld = h.result_device()
        assert ptr and ld == 7400
        _same(h.result_to_host(), genea140_exact)
    finally:
        h.close()


@pytest.mark.parametrize("panel", [1, 3, 64, 65])
def test_genea140_column_panels(gen, genea140, genea140_exact, monkeypatch, panel):
    """7,399 founders in panels of 1, 3 (a ragged last panel of 1), 64 (ragged: 39; every panel starts on a multiple of 8 columns:
    16-byte result stores) and 65 columns (ragged: 54; element stores), all panels in one launch through grid dimension y."""
    monkeypatch.setenv("GENPHI_DIST_PANEL", str(panel))
    ped, pro, anc = genea140
    h = gen.DistPlan(*_args(ped), pro, anc)
    try:
        h.compute()
        st = h.stats()
        assert st["panel_cols"] == panel
        assert st["launches"] < 2 * (7399 // panel + 1)            # fewer launches than panels x lists: several panels per launch
        _same(h.result_to_host(), genea140_exact)
    finally:
        h.close()


@pytest.mark.parametrize("panel,group", [(100, 1), (100, 7), (104, 5)])
def test_genea140_panels_per_launch(gen, genea140, genea140_exact, monkeypatch, panel, group):
    """Panels of 100 (element stores) and 104 columns (16-byte stores), one, seven and five per launch; the last launch is short
    and the last panel ragged (99 and 15 columns)."""
    monkeypatch.setenv("GENPHI_DIST_PANEL", str(panel))
    monkeypatch.setenv("GENPHI_DIST_PANELS_PER_LAUNCH", str(group))
    ped, _, _ = genea140
    _same(gen.meioses(ped), genea140_exact)


def test_hand_built_quirks(gen):
    """A repeated proband, probands with children (one three cuts above the last), probands that are requested ancestors (0), a
    duplicated ancestor (equal columns), an unrelated ancestor (all -1), one-parent members, and 12 -> 1 in 3 steps past the
    requested ancestor 3 (4 steps through it)."""
    ped = quirk_pedigree(gen)
    out = gen.meioses(ped, QUIRK_PRO, QUIRK_ANC)
    _same(out, QUIRK_MEIOSES)
    assert np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[0], out[3]) and np.all(out[:, 6] == -1)
    _same(out, MO.meioses_literal(*_args(ped), QUIRK_PRO, QUIRK_ANC))
    _same_matrix(gen.findMRCA(ped, [12, 7, 12]), [12, 7, 12], MO.find_mrca_literal(*_args(ped), [12, 7, 12]))
    assert gen.findMRCA(ped, [12, 7, 12]).ancestors.tolist() == [3, 4]        # 1 and 2 are common, and parents of the common 3
    # probands that are unrelated to every ancestor: rows of -1 beside computed rows
    _same(gen.meioses(ped, [10, 12, 11, 5], [3, 4]), np.array([[-1, -1], [3, 2], [-1, -1], [-1, -1]], dtype=np.int16))
    # 8 is an ancestor of 12: not a common ancestor of the two (ancestors are strict)
    _same_matrix(gen.findMRCA(ped, [12, 8]), [12, 8], MO.find_mrca_literal(*_args(ped), [12, 8]))
    _same(gen.findFounders(ped, [12, 8]), np.array([1, 2, 5]), np.int64)
    _same(gen.findFounders(ped, [1, 3]), np.zeros(0, dtype=np.int64), np.int64)   # a founder listed in IDs is not its own ancestor


def test_shortcut_past_requested_ancestors(gen):
    ind, fa, mo = shortcut_pedigree()
    ped = _ped(gen, ind, fa, mo)
    _same(gen.meioses(ped, SHORTCUT_PRO, SHORTCUT_ANC), SHORTCUT_MEIOSES)
    assert gen.findDistance(ped, [5, 3], 1) == 4 and gen.findDistance(ped, [4, 4], 4) == 0


def test_errors_and_empty_results(gen, genea140):
    ped, pro, anc = genea140
    p0, p1, a0 = int(pro[0]), int(pro[1]), int(anc[0])
    for call in (lambda: gen.meioses(ped, pro=[p0, 10 ** 9]), lambda: gen.meioses(ped, ancestors=[a0, 10 ** 9]),
                 lambda: gen.findMRCA(ped, [10 ** 9, p0]), lambda: gen.findMRCA(ped, [p0, p1, 10 ** 9]),
                 lambda: gen.findFounders(ped, [p0, 10 ** 9]), lambda: gen.findDistance(ped, [10 ** 9, p0], a0),
                 lambda: gen.findDistance(ped, [p0, 10 ** 9], a0), lambda: gen.findDistance(ped, [p0, p1], 10 ** 9),
                 lambda: gen._findMinDistanceMRCA(ped, [p0, 10 ** 9]), lambda: gen.ancestor(ped, 10 ** 9)):
        with pytest.raises(KeyError):
            call()
    own = gen.ancestor(ped, p0)
    stranger = int(np.setdiff1d(anc, own)[0])
    with pytest.raises(ValueError):
        gen.findDistance(ped, [p0, p1], stranger)                    # not an ancestor of the first
    with pytest.raises(ValueError):
        gen.findDistance(ped, [p0, p0], p1)
    with pytest.raises(ValueError):
        gen._findMinDistanceMRCA(ped, pro)                           # all 140 have no common ancestor
    for ids in ([p0], []):
        with pytest.raises(IndexError):
            gen.findDistance(ped, ids, a0)
        with pytest.raises(IndexError):
            gen._findMinDistanceMRCA(ped, ids)
    assert gen.meioses(ped, pro=[], ancestors=anc[:5]).shape == (0, 5)
    assert gen.meioses(ped, pro=pro[:4], ancestors=[]).shape == (4, 0)
    m = gen.findMRCA(ped, pro)
    assert m.ancestors.shape == (0,) and m.meioses.shape == (140, 0) and m.meioses.dtype == np.int64
    one = gen.findMRCA(ped, [p0])                                    # one individual: its parents
    assert sorted(one.ancestors.tolist()) == sorted(int(x) for x in (ped[p0].father.ID, ped[p0].mother.ID))
    assert one.meioses.tolist() == [[1, 1]]


@pytest.mark.parametrize("n_anc", [13, 63, 130])
def test_genea140_mixed_lists(gen, genea140, n_anc):
    """Unsorted, repeated, non-leaf and founder probands; non-founder, duplicated and proband ancestors."""
    ped, _, _ = genea140
    pro, anc = _mixed_lists(ped, gen, np.random.default_rng(n_anc), n_anc)
    out = gen.meioses(ped, pro, anc)
    _same(out, MO.meioses_exact(*_args(ped), pro, anc))
    _same(out, MO.meioses_literal(*_args(ped), pro, anc))


def test_one_parent_synthetic(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, spro = _one_parent_synth(synth)
    ped = _ped(gen, ind, fa, mo, sex)
    pro, anc = _mixed_lists(ped, gen, np.random.default_rng(5), 21)
    _same(gen.meioses(ped, pro, anc), MO.meioses_exact(*_args(ped), pro, anc))
    anc = np.setdiff1d(ped.ind, gen.pro(ped))[::5]                   # every fifth individual with children: all depths
    _same(gen.meioses(ped, gen.pro(ped), anc), MO.meioses_exact(*_args(ped), gen.pro(ped), anc))
    for ids in (spro[:2], spro[[3, 9, 200]], spro[:40]):
        _same_matrix(gen.findMRCA(ped, ids), ids, MO.find_mrca_exact(*_args(ped), ids))


def test_unsorted_ranks(gen):
    """sort=false: ranks follow a parents-first file order, not the depth."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, spro = _one_parent_synth(synth)
    ind, fa, mo, sex = synth.parents_first_shuffle(ind, fa, mo, sex, seed=3)
    ped = _ped(gen, ind, fa, mo, sex, sort=False)
    pro, anc = _mixed_lists(ped, gen, np.random.default_rng(9), 17)
    _same(gen.meioses(ped, pro, anc), MO.meioses_exact(*_args(ped), pro, anc))
    _same_matrix(gen.findMRCA(ped, spro[:3]), spro[:3], MO.find_mrca_exact(*_args(ped), spro[:3]))


def test_probands_all_founders(gen):
    """Zero level steps: only founders among the probands."""
    ped = quirk_pedigree(gen)
    _same(gen.meioses(ped, [1, 2, 10, 1], [1, 10, 3]), np.array([[0, -1, -1], [-1, -1, -1], [-1, 0, -1], [0, -1, -1]], dtype=np.int16))


@pytest.mark.parametrize("generations", [256, 300, 1000])
def test_deeper_than_255_steps(gen, generations):
    """255, 299 and 999 steps: distances an 8-bit row could not hold; the rows are 16 bits wide."""
    ind, fa, mo = doubling_chain(generations)
    ped = _ped(gen, ind, fa, mo)
    pro = [2 * generations, 2 * generations - 1, 2 * generations - 2, 7]
    anc = [1, 2, 5, 2 * generations - 1]
    h = gen.DistPlan(*_args(ped), pro, anc)
    try:
        h.compute()
        assert h.stats()["row_bits"] == 16
        out = h.result_to_host()
    finally:
        h.close()
    _same(out, MO.meioses_exact(*_args(ped), pro, anc))
    g = generations
    assert out.tolist() == [[g - 1, g - 1, g - 3, -1], [g - 1, g - 1, g - 3, 0], [g - 2, g - 2, g - 4, -1], [3, 3, 1, -1]]
    m = gen.findMRCA(ped, [2 * g, 2 * g - 1])
    assert m.ancestors.tolist() == [2 * g - 3, 2 * g - 2] and m.meioses.tolist() == [[1, 1], [1, 1]]


def test_depth_limit(gen):
    """32,767 steps is the deepest sweep a signed 16-bit distance covers: computed; one more is an error at create."""
    g = 32768
    ind, fa, mo = doubling_chain(g)
    out = gen.meioses(_ped(gen, ind, fa, mo), [2 * g, 2 * g - 2], [1, 4, 2 * g])
    assert out.tolist() == [[32767, 32766, 0], [32766, 32765, -1]]
    ind, fa, mo = doubling_chain(g + 1)
    with pytest.raises(ValueError, match="32767"):
        gen.meioses(_ped(gen, ind, fa, mo), [2 * g + 2], [1])


def test_two_lines_from_one_couple(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, tips = synth.chain_two_lines(300)
    ped = _ped(gen, ind, fa, mo, sex)
    m = gen.findMRCA(ped, tips)
    _same_matrix(m, tips, MO.find_mrca_exact(*_args(ped), tips))
    assert m.ancestors.tolist() == [1, 2] and m.meioses.tolist() == [[300, 300], [300, 300]]
    assert gen.findDistance(ped, tips, 1) == 600 and gen._findMinDistanceMRCA(ped, tips) == 600


def test_cfg3_all_founders(gen, cfg3):
    """cfg3: 1e4 probands x 6,633 founders; 64 sampled proband rows against the exact search."""
    ped, pro = cfg3
    anc = gen.founder(ped)
    assert len(anc) == 6633
    sample = np.random.default_rng(3).choice(len(pro), 64, replace=False)
    out = gen.meioses(ped, pro, anc)
    assert out.shape == (10_000, 6633)
    _same(out[sample], MO.meioses_exact(*_args(ped), pro, anc, sample=sample))


@pytest.mark.parametrize("n,n_common,n_mrca", [(2, 25_254, 829), (16, 19_260, 1_433), (256, 0, 0)])
def test_cfg3_findMRCA(gen, cfg3, n, n_common, n_mrca):
    ped, pro = cfg3
    ref = MO.find_mrca_exact(*_args(ped), pro[:n])
    assert (ref[2], len(ref[0])) == (n_common, n_mrca)
    m = gen.findMRCA(ped, pro[:n])
    _same_matrix(m, pro[:n], ref)
    assert m.meioses.shape == (n, n_mrca)


def test_c_abi_from_plain_ctypes(gen, genea140, genea140_exact):
    """create, compute, result_to_host, destroy through ctypes alone; compute twice gives the same bits; destroy without compute;
    the host glue."""
    from genlib_jl_amd import _capi
    ped, pro, anc = genea140
    L = ctypes.CDLL(_capi.LIB_PATH)
    P64, P16 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int16)
    arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (ped.ind, ped.father, ped.mother, pro, anc)]
    ptr = [a.ctypes.data_as(P64) for a in arrs]
    n = [ctypes.c_int64(len(a)) for a in arrs]
    L.genphi_dist_destroy.restype = None
    L.genphi_dist_destroy.argtypes = [ctypes.c_void_p]
    L.genphi_free.restype = None
    L.genphi_free.argtypes = [ctypes.c_void_p]
    h = ctypes.c_void_p()
    assert L.genphi_dist_create(n[0], ptr[0], ptr[1], ptr[2], n[3], ptr[3], n[4], ptr[4], ctypes.byref(h)) == 0
    L.genphi_dist_destroy(h)                                         # never computed
    h = ctypes.c_void_p()
    assert L.genphi_dist_create(n[0], ptr[0], ptr[1], ptr[2], n[3], ptr[3], n[4], ptr[4], ctypes.byref(h)) == 0
    outs = []
    for _ in range(2):
        assert L.genphi_dist_compute(h, ctypes.c_int32(-1)) == 0
        out = np.full((len(pro), len(anc)), 7, dtype=np.int16)
        assert L.genphi_dist_result_to_host(h, out.ctypes.data_as(P16)) == 0
        outs.append(out)
    bits, launches = ctypes.c_int32(), ctypes.c_int64()
    assert L.genphi_dist_stats(h, None, None, None, None, ctypes.byref(bits), ctypes.byref(launches)) == 0
    assert bits.value == 16 and launches.value > 0
    L.genphi_dist_destroy(h)
    _same(outs[0], outs[1])
    _same(outs[0], genea140_exact)
    bad = np.array([10 ** 9], dtype=np.int64)
    h = ctypes.c_void_p()
    assert L.genphi_dist_create(n[0], ptr[0], ptr[1], ptr[2], ctypes.c_int64(1), bad.ctypes.data_as(P64), n[4], ptr[4], ctypes.byref(h)) == 1       # GENPHI_ERR_UNKNOWN_ID
    assert not h.value
    cnt, res = ctypes.c_int64(), P64()
    assert L.genphi_ancestors(n[0], ptr[0], ptr[1], ptr[2], ctypes.c_int64(2), ptr[3], ctypes.byref(cnt), ctypes.byref(res)) == 0
    got = np.ctypeslib.as_array(res, shape=(cnt.value,)).copy()
    L.genphi_free(res)
    assert got.tolist() == MO.ancestor_literal(MO._parents(*_args(ped)), [int(pro[0]), int(pro[1])])
