"""gen.simuUniqueness without a GPU: the reference of tests/uniqueness_oracle.py on hand-made labels and its invariants on a real
pedigree, the host plan of gen.UniquenessPlan against gen.IdentityPlan's on probands + others, every argument error and limit of the
definition (include/genphi.h, genphi_unique_*) with its text, the derived fields of gen.SimuUniqueness from hand-made integer tables,
and csrc/unique.h as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (tests/unique_check.cpp)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from random_pedigree import random_pedigree
from uniqueness_oracle import UniqueVector, check_founders_and_children, check_lumped, check_rows, shares, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SUMMARY = re.compile(r"^unique check: (\d+) chunk cases, (\d+) chunks walked, (\d+) plans, (\d+) overlaps folded, (\d+) lists with repeats; (\d+) violations$", re.M)

IND = np.arange(1, 10, dtype=np.int64)
FA = np.array([0, 0, 1, 1, 3, 3, 0, 5, 0], dtype=np.int64)
MO = np.array([0, 0, 2, 2, 4, 3, 4, 7, 0], dtype=np.int64)
MAX_CHUNK = 1216                             # csrc/unique.h: UNIQUE_MAX_CHUNK


def _default_chunk():
    """UNIQUE_DEFAULT_CHUNK of csrc/unique.h: the measured winner of 640 and 1,216."""
    text = open(os.path.join(ROOT, "genlib.jl_amd", "csrc", "unique.h")).read()
    m = re.search(r"constexpr int64_t UNIQUE_DEFAULT_CHUNK = (\w+);", text)
    assert m, "UNIQUE_DEFAULT_CHUNK"
    value = MAX_CHUNK if m.group(1) == "UNIQUE_MAX_CHUNK" else int(m.group(1))
    assert value in (640, 1216)
    return value


def _rule(n_labels, arg):
    """(chunk_labels, chunks, lds_bytes) as csrc/unique.h gives them."""
    lc = min(n_labels, MAX_CHUNK, (arg + 63) // 64 * 64 if arg else _default_chunk())
    return lc, -(-n_labels // lc), 256 * (((lc + 1) // 2) | 1)


def _ped(gen, ind, fa, mo):
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)


def _founders(n):
    """n unrelated founders."""
    return np.arange(1, n + 1, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)


def test_the_oracle_on_hand_made_labels():
    """Two probands and two others, five labels, four simulations.
    s = 0: the probands carry (0, 1), (2, 1); the others (0, 0), (4, 4).     s = 1: (0, 0), (0, 1); the others (4, 3), (1, 2).
    s = 2: everyone (1, 1).                                                   s = 3: (3, 4), (3, 3); the others (3, 3), (0, 0)."""
    pop = np.array([[[0, 0, 1, 3], [1, 0, 1, 4]],
                    [[2, 0, 1, 3], [1, 1, 1, 3]],
                    [[0, 4, 1, 3], [0, 3, 1, 3]],
                    [[4, 1, 1, 0], [4, 2, 1, 0]]], dtype=np.int32)
    c1 = shares(pop, 5)
    assert c1.T.tolist() == [[2, 2, 1, 0, 1], [2, 2, 1, 1, 1], [0, 4, 0, 0, 0], [1, 0, 0, 3, 1]]
    alleles, autozygous = tables(pop, 2, 5)
    # proband 0: s0 (0: 2, 1: 2), s1 (0, 0): 2 once, s2 (1, 1): 4 once, s3 (3: 3, 4: 1)
    assert alleles.tolist() == [[1, 3, 1, 1], [1, 3, 1, 1]] and autozygous.tolist() == [[0, 1, 0, 1], [0, 0, 1, 1]]
    check_rows(alleles, autozygous, 4, 4)
    alone, alone_z = tables(pop[:2], 2, 5)                               # the probands without the others
    assert alone.tolist() == [[2, 4], [2, 4]] and alone_z.tolist() == [[0, 2], [0, 2]]
    for k in (1, 2, 3):
        cut, cut_z = tables(pop, 2, 5, max_share=k)
        assert cut.shape == (2, k)
        check_lumped(alleles, cut)
        check_lumped(autozygous, cut_z)
        check_rows(cut, cut_z, 4, 4)
    assert tables(pop, 2, 5, max_share=1)[0].tolist() == [[6], [6]]
    assert np.array_equal(tables(pop, 2, 5, max_share=4)[0], alleles) and np.array_equal(tables(pop, 2, 5, max_share=9)[0], alleles)
    # invariant 6 on the hand-made labels: with the others the cumulated shares do not rise
    wide = np.zeros((2, 4), dtype=np.int64)
    wide[:, :2] = alone
    assert np.all(np.cumsum(alleles, axis=1) <= np.cumsum(wide, axis=1))


def test_invariants_on_the_reference(gen):
    """Invariants 1, 6, 7 and 8 on the reference itself, and the lists as sets."""
    rng = np.random.default_rng(5)
    ind, fa, mo, _ = random_pedigree(rng, 300, p_founder=0.08, p_one_parent=0.1, p_selfing=0.05, max_back=25)
    pro = rng.choice(ind[100:], size=14, replace=False).astype(np.int64)
    pro[9], pro[13], pro[4] = pro[1], pro[1], ind[0]
    parents_of = np.unique(np.concatenate([fa[pro - 1], mo[pro - 1]]))
    others = np.concatenate([np.setdiff1d(ind[60:], pro)[::23][:8], parents_of[parents_of > 0][:6], pro[:2]]).astype(np.int64)
    S = 1000
    plain = UniqueVector(ind, fa, mo, pro, None, S, 31)
    alleles, autozygous = plain.at(S)
    assert plain.n == plain.n_pop == 12 and alleles.shape == (12, 12) and set(plain.ids.tolist()) == set(pro.tolist())
    check_rows(alleles, autozygous, S, 12)
    assert autozygous.any() and alleles[:, 1:].any()
    ref = UniqueVector(ind, fa, mo, pro, others, S, 31)
    a2, z2 = ref.at(S)
    assert ref.n == 12 and ref.n_pop == 12 + len(np.setdiff1d(others, pro)) and np.array_equal(np.sort(ref.pop_ids[12:]), np.setdiff1d(others, pro))
    check_rows(a2, z2, S, ref.n_pop)
    lone, children = check_founders_and_children(a2, z2, ref.ids, ref.pop_ids, ind, fa, mo, S)
    assert lone >= 0 and children >= 1
    # 6: keyed by ID (the two plans order their rows alike here, asserted)
    at = {int(x): i for i, x in enumerate(plain.ids.tolist())}
    rows = [at[int(x)] for x in ref.ids.tolist()]
    for wide, narrow in ((a2, alleles[rows]), (z2, autozygous[rows])):
        pad = np.zeros(wide.shape, dtype=np.int64)
        pad[:, : narrow.shape[1]] = narrow
        assert np.all(np.cumsum(wide, axis=1) <= np.cumsum(pad, axis=1))
    assert np.any(np.cumsum(a2, axis=1)[:, 0] < alleles[rows][:, 0])
    other = UniqueVector(ind, fa, mo, np.concatenate([pro[::-1], pro[:5]]), np.concatenate([others, others[::-1]]), S, 31)
    assert np.array_equal(other.ids, ref.ids)
    for a, b in zip(other.at(S), (a2, z2)):
        assert np.array_equal(a, b)
    for k in (1, 2, 8):
        for cut, full in zip(ref.at(S, max_share=k), (a2, z2)):
            check_lumped(full, cut)


def _check_plan(gen, ind, fa, mo, pro, others, **kw):
    h = gen.UniquenessPlan(ind, fa, mo, pro, others, simul_no=64, seed=1, **kw)
    g = gen.IdentityPlan(ind, fa, mo, np.concatenate([pro, others]).astype(np.int64), simul_no=64, seed=1)
    try:
        assert (h.n_live, h.levels, h.n_labels, h.planes, h.n_pro) == (g.n_live, g.levels, g.n_labels, g.planes, g.n_pro)
        assert np.array_equal(h.rows_per_level(), g.rows_per_level())
        got = h.alleles()
        assert got.dtype == np.int64 and np.array_equal(got, g.alleles())
        st, gs = h.stats(), g.stats()
        assert st["sweep_ms"] == 0.0 and st["count_ms"] == 0.0 and st["count_bytes"] == 0.0
        assert (st["planes"], st["levels"], st["panel_cols"], st["panels"]) == (gs["planes"], gs["levels"], gs["panel_cols"], gs["panels"])
        n, n_pop = len(np.unique(pro)), len(np.union1d(pro, others))
        assert (st["n"], st["n_pop"]) == (n, n_pop) == (h.n, h.n_pop)
        ids = h.probands()
        assert ids.dtype == np.int64 and len(ids) == n and np.array_equal(np.sort(ids), np.unique(pro))
        assert np.array_equal(ids, UniqueVector(ind, fa, mo, pro, others, 1, 1).ids)                 # ascending row: level, then position
        return h.n_labels, st
    finally:
        h.close()
        g.close()


def test_plan_is_the_identity_plan_on_probands_and_others(gen):
    ped = gen.genealogy(gen.geneaJi)
    pro = gen.pro(ped)
    n_labels, st = _check_plan(gen, ped.ind, ped.father, ped.mother, pro, np.zeros(0, dtype=np.int64))
    assert (st["chunk_labels"], st["chunks"], st["lds_bytes"], st["columns"]) == (n_labels, 1, 256 * (((n_labels + 1) // 2) | 1), len(pro))
    _check_plan(gen, ped.ind, ped.father, ped.mother, pro[[2, 0, 2]], pro[[1, 1, 2]])
    rng = np.random.default_rng(99)
    seen = set()
    for k in range(60):
        ind, fa, mo, _ = random_pedigree(rng, int(rng.integers(2, 900)), p_founder=0.25, p_one_parent=0.1, p_selfing=0.03, max_back=40)
        order = rng.permutation(ind)
        n_pro = int(rng.integers(1, min(10, len(ind))))
        pro = rng.choice(order[:n_pro], size=n_pro + int(rng.integers(0, 3)), replace=True).astype(np.int64)
        others = rng.choice(order, size=int(rng.integers(0, 6)), replace=True).astype(np.int64) if k % 3 else order[:0]       # may meet the probands
        arg, ms = [0, 64, 65, 128][k % 4], [0, 1, 2, 100][k % 4]
        n_labels, st = _check_plan(gen, ind, fa, mo, pro, others, chunk_labels=arg, max_share=ms)
        assert (st["chunk_labels"], st["chunks"], st["lds_bytes"]) == _rule(n_labels, arg)
        assert st["columns"] == (min(st["n_pop"], ms) if ms else st["n_pop"])
        seen.add(st["chunks"])
    assert len(seen) >= 3


def test_planned_shapes(gen):
    h = gen.UniquenessPlan(IND, FA, MO, [8, 6, 8], [9, 9, 6], simul_no=5000, seed=3, panel_cols=1000, chunk_labels=1, max_share=2)
    try:
        assert (h.n_live, h.levels, h.n_labels, h.planes, h.n_pro, h.simul_no, h.seed) == (9, 4, 7, 3, 6, 5000, 3)
        assert h.alleles().tolist() == [[1, 0], [1, 1], [2, 0], [2, 1], [7, 0], [9, 0], [9, 1]]
        assert (h.n, h.n_pop, h.columns) == (2, 3, 2) and h.probands().tolist() == [6, 8]
        st = h.stats()
        assert (st["panel_cols"], st["panels"], st["chunk_labels"], st["chunks"], st["lds_bytes"]) == (1024, 5, 7, 1, 256 * 5)
    finally:
        h.close()


def test_argument_errors(gen):
    ok = dict(pro_ids=[8, 6], other_ids=[9], simul_no=10, seed=3)

    def plan(**kw):
        a = {**ok, **kw}
        gen.UniquenessPlan(a.pop("ind", IND), a.pop("fa", FA), a.pop("mo", MO), **a).close()

    plan()
    plan(other_ids=None)
    plan(other_ids=[])
    plan(simul_no=1 << 24)
    plan(simul_no=1, panel_cols=7, chunk_labels=7, max_share=7)
    plan(chunk_labels=2**31 - 1, max_share=2**31 - 1)
    plan(pro_ids=[8, 8, 6], other_ids=[9, 9, 7])
    for pro, others in (([8, 6], [6]), ([8, 6], [9, 8, 9]), ([1], [1]), ([8, 6, 8], [7, 6])):                  # in both lists: a proband
        plan(pro_ids=pro, other_ids=others)
    with pytest.raises(KeyError):
        plan(pro_ids=[8, 99])
    with pytest.raises(KeyError):
        plan(other_ids=[99])
    with pytest.raises(KeyError):
        plan(pro_ids=[0])
    for kw, text in ((dict(simul_no=0), r"simulNo = 0 is outside 1 \.\. 2\^24"), (dict(simul_no=-5), "simulNo = -5 is outside"),
                     (dict(simul_no=(1 << 24) + 1), "simulNo = 16777217 is outside"), (dict(pro_ids=[]), "gen.simuUniqueness: no probands"),
                     (dict(pro_ids=[], other_ids=[]), "no probands"), (dict(panel_cols=-1), "panel_cols is 0 .the default rule. or positive"),
                     (dict(chunk_labels=-1), "chunk_labels is 0 .the default rule. or positive"),
                     (dict(max_share=-1), "max_share is 0 .every share has its column. or positive")):
        with pytest.raises(ValueError, match=text):
            plan(**kw)
    with pytest.raises(Exception, match="duplicate"):
        plan(ind=np.array([1, 2, 3, 4, 5, 6, 7, 8, 1]))
    with pytest.raises(Exception, match="rank order"):
        plan(fa=np.array([8, 0, 1, 1, 3, 3, 0, 5, 0]))
    # the C entry point itself: NULL out, NULL lists, negative sizes, NULL handles
    L = gen._capi.lib()
    i64 = ctypes.POINTER(ctypes.c_int64)
    pro, con = np.array([8], dtype=np.int64), np.array([9], dtype=np.int64)
    ped = [len(IND), IND.ctypes.data_as(i64), FA.ctypes.data_as(i64), MO.ctypes.data_as(i64)]
    h = ctypes.c_void_p()
    ARG = gen._capi.GENPHI_ERR_ARG
    L.genphi_last_error.restype = ctypes.c_char_p
    assert L.genphi_unique_create(*ped, 1, pro.ctypes.data_as(i64), 1, con.ctypes.data_as(i64), 10, 3, 0, 0, 0, None) == ARG
    assert b"genphi_unique_create: out is NULL" in L.genphi_last_error()
    assert L.genphi_unique_create(*ped, 1, pro.ctypes.data_as(i64), 1, None, 10, 3, 0, 0, 0, ctypes.byref(h)) == ARG and not h.value
    assert b"genphi_unique_create: bad sizes or NULL arrays" in L.genphi_last_error()
    assert L.genphi_unique_create(*ped, 1, None, 0, None, 10, 3, 0, 0, 0, ctypes.byref(h)) == ARG and not h.value
    assert L.genphi_unique_create(*ped, -1, pro.ctypes.data_as(i64), 0, None, 10, 3, 0, 0, 0, ctypes.byref(h)) == ARG and not h.value
    assert L.genphi_unique_create(*ped, 1, pro.ctypes.data_as(i64), -1, con.ctypes.data_as(i64), 10, 3, 0, 0, 0, ctypes.byref(h)) == ARG and not h.value
    assert L.genphi_unique_create(*ped, 0, None, 1, con.ctypes.data_as(i64), 10, 3, 0, 0, 0, ctypes.byref(h)) == ARG and not h.value
    assert b"gen.simuUniqueness: no probands" in L.genphi_last_error()
    assert L.genphi_unique_create(*ped, 1, pro.ctypes.data_as(i64), 0, None, 10, 3, 0, 0, 0, ctypes.byref(h)) == 0 and h.value
    n = ctypes.c_int64()
    assert L.genphi_unique_probands(h, ctypes.byref(n), None) == 0 and n.value == 1
    L.genphi_unique_destroy(h)
    assert L.genphi_unique_levels(None, None, None, None) == ARG and L.genphi_unique_alleles(None, None, None, None, None) == ARG
    assert L.genphi_unique_probands(None, None, None) == ARG and L.genphi_unique_compute(None, 0) == ARG
    assert L.genphi_unique_stats(None, *([None] * 14)) == ARG
    for name in ("alleles", "autozygous"):
        assert getattr(L, "genphi_unique_%s_to_host" % name)(None, None) == ARG
    L.genphi_unique_destroy(None)
    hp = gen.UniquenessPlan(IND, FA, MO, [8, 6], simul_no=10, seed=3)
    for fn in (hp.alleles_to_host, hp.autozygous_to_host):
        with pytest.raises(ValueError, match="nothing computed"):
            fn()
    hp.close()
    ped = _ped(gen, IND, FA, MO)
    with pytest.raises(ValueError):
        gen.simuUniqueness(ped, pro=[])
    with pytest.raises(KeyError):
        gen.simuUniqueness(ped, pro=[77])
    with pytest.raises(KeyError):
        gen.simuUniqueness(ped, pro=[8], others=[77])
    with pytest.raises(ValueError):
        gen.simuUniqueness(ped, simulNo=0)
    with pytest.raises(ValueError):
        gen.simuUniqueness(ped, maxShare=-1)
    with pytest.raises(TypeError):
        gen.simuUniqueness(ped, controls=[1])
    h1, h2 = gen.UniquenessPlan(IND, FA, MO, [8]), gen.UniquenessPlan(IND, FA, MO, [8])
    assert 0 <= h1.seed < 2**64 and h1.seed != h2.seed and h1.simul_no == 5000
    h1.close()
    h2.close()


def test_the_limits_on_unrelated_founders(gen):
    """A population of 65,535 is taken and 65,536 refused, whoever of them is a proband; repeats and an other that is a proband do not
    count.  With 65,535 columns 32,768 probands are 2^31 - 32,768 cells and are taken, 32,769 are 2^31 + 32,767 and are refused with
    the advice to pass a smaller maxShare, which then lets them in."""
    ind, fa, mo = _founders(65540)
    h = gen.UniquenessPlan(ind, fa, mo, ind[:5], ind[5:65535], simul_no=64, seed=1)
    try:
        assert (h.n, h.n_pop, h.columns, h.n_labels, h.planes) == (5, 65535, 65535, 131070, 17)
        st = h.stats()
        assert (st["chunk_labels"], st["chunks"], st["lds_bytes"]) == _rule(131070, 0)
    finally:
        h.close()
    gen.UniquenessPlan(ind, fa, mo, np.concatenate([ind[:5], ind[:5]]), np.concatenate([ind[:65535], ind[:40]]), simul_no=64, seed=1, max_share=5).close()
    for pro, others in ((ind[:5], ind[5:65536]), (ind[:65536], None), (ind[:1], ind[:65536])):
        with pytest.raises(ValueError, match="65536 distinct probands and others; at most 65,535 are counted"):
            gen.UniquenessPlan(ind, fa, mo, pro, others, simul_no=64, seed=1, max_share=1)
    h = gen.UniquenessPlan(ind, fa, mo, ind[:32768], ind[32768:65535], simul_no=64, seed=1)
    try:
        assert (h.n, h.n_pop, h.columns) == (32768, 65535, 65535) and h.n * h.columns == 2**31 - 32768
    finally:
        h.close()
    with pytest.raises(ValueError, match=r"32769 probands x 65535 columns are more than 2\^31 - 1 cells; pass a smaller maxShare"):
        gen.UniquenessPlan(ind, fa, mo, ind[:32769], ind[32769:65535], simul_no=64, seed=1)
    with pytest.raises(ValueError, match="pass a smaller maxShare"):
        gen.UniquenessPlan(ind, fa, mo, ind[:65535], simul_no=64, seed=1, max_share=32769)
    h = gen.UniquenessPlan(ind, fa, mo, ind[:65535], simul_no=64, seed=1, max_share=32768)
    try:
        assert (h.n, h.n_pop, h.columns) == (65535, 65535, 32768) and h.n * h.columns == 2**31 - 32768
    finally:
        h.close()


def test_symbols_are_exported_declared_and_bound(gen):
    from genlib_jl_amd import _capi
    header = open(os.path.join(ROOT, "include", "genphi.h")).read()
    L = ctypes.CDLL(_capi.LIB_PATH)
    names = ["genphi_unique_" + n for n in ("create", "levels", "alleles", "probands", "compute", "alleles_to_host", "autozygous_to_host", "stats", "destroy")]
    for name in names:
        assert hasattr(L, name) and name in _capi.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, header), name
    assert sum(n.startswith("genphi_unique_") for n in _capi.EXPORTED_SYMBOLS) == 9
    assert len(_capi.lib().genphi_unique_create.argtypes) == 14 and len(_capi.lib().genphi_unique_stats.argtypes) == 15
    assert gen.UniquenessPlan is _capi.UniquenessPlan and gen.simuUniqueness.__doc__ and gen.SimuUniqueness.__doc__
    text = header[header.index("gen.simuUniqueness"):header.index("typedef struct genphi_unique")]
    for k in range(1, 9):
        assert re.search(r"^ \*\s+%d\. " % k, text, re.M), k
    for what in ("uniqueness within groups", "sole carrier", "linked loci", "more than one device"):
        assert what in text, what
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"unique.hip"' in entry and '"unique.h"' in entry


def test_SimuUniqueness_derived_fields(gen):
    """The shares from hand-made integer tables, S = 10, three probands in a population of 4."""
    alleles = np.array([[20, 0, 0, 0], [4, 6, 2, 0], [4, 6, 0, 4]], dtype=np.int32)
    autozygous = np.array([[0, 0, 0, 0], [2, 0, 2, 0], [0, 3, 0, 0]], dtype=np.int32)
    r = gen.SimuUniqueness(np.array([7, 8, 9]), 4, alleles, autozygous, 10, 1)
    assert not r.lumped and r.n_pop == 4 and r.simulNo == 10 and r.seed == 1
    assert r.copies.dtype == np.int64 and r.copies.tolist() == [[20, 0, 0, 0], [6, 6, 4, 0], [4, 9, 0, 4]]
    assert r.uniqueness.dtype == np.float64 and r.uniqueness.tolist() == [1.0, 6 / 20, 4 / 20]
    assert r.at_risk.tolist() == [2.0, 0.4, 0.4]
    assert r.share_hist.shape == (3, 4) and r.share_hist[1].tolist() == [6 / 20, 6 / 20, 4 / 20, 0.0]
    assert r.mean_share.tolist() == [1.0, (6 + 12 + 12) / 20, (4 + 18 + 16) / 20]
    assert r.ranking().tolist() == [0, 1, 2] and r.ranking(2).tolist() == [0, 1] and r.ranking(0).tolist() == []
    assert "3 probands" in repr(r) and "population of 4" in repr(r)
    tie = gen.SimuUniqueness(np.array([7, 8, 9]), 4, alleles[[1, 0, 1]], autozygous[[1, 0, 1]], 10, 1)
    assert tie.ranking().tolist() == [1, 0, 2]                                                       # ties by position
    cut = gen.SimuUniqueness(np.array([7, 8, 9]), 5, alleles, autozygous, 10, 1)                     # a population of 5 in 4 columns
    assert cut.lumped and cut.mean_share is None and cut.uniqueness.tolist() == r.uniqueness.tolist()


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_unique_h_as_a_stand_alone_program(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "unique_check")
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra"] + flags + [os.path.join(ROOT, "tests", "unique_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if san is not None and build.returncode != 0 and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("this toolchain has no -fsanitize=" + san)
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    if san is not None and run.returncode != 0 and not run.stdout and any(
            t in run.stderr for t in ("unexpected memory mapping", "runtime does not come first", "failed to intercept", "ReserveShadowMemoryRange failed")):
        pytest.skip("the sanitizer runtime does not start in this environment: " + run.stderr[:200])
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    m = SUMMARY.search(run.stdout)
    assert m, run.stdout[-1500:]
    cases, walked, plans, overlaps, repeats, violations = (int(v) for v in m.groups())
    assert violations == 0 and cases >= 250 and walked > 10**7 and plans == 20000 and overlaps > 1000 and repeats > 1000
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
