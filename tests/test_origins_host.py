"""gen.simuOrigins without a GPU: the reference of tests/origins_oracle.py on hand-made labels with every cell written out, its
invariants on a random pedigree (against the literal count over pairs, tests/ident_oracle.py's identity states and
tests/carriers_oracle.py's tables), the host plan of gen.OriginsPlan against gen.IdentityPlan's, every argument error and limit of the
definition (include/genphi.h, genphi_origin_*), the shares of gen.SimuOrigins from hand-made integer tables, and csrc/origin.h as a
stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (tests/origin_check.cpp)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from carriers_oracle import tables as carry_tables
from ident_oracle import counts_of
from origins_oracle import OriginVector, check_invariants, exact_kinship, expected_frequency, matches_by_pairs, merge, pair_index, tables
from random_pedigree import random_pedigree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SUMMARY = re.compile(r"^origin check: (\d+) chunk cases, (\d+) chunks walked, (\d+) plans, (\d+) conflicts refused, (\d+) groups out of range refused, "
                     r"(\d+) lists with repeats, (\d+) with ungrouped probands; (\d+) violations$", re.M)

IND = np.arange(1, 10, dtype=np.int64)
FA = np.array([0, 0, 1, 1, 3, 3, 0, 5, 0], dtype=np.int64)
MO = np.array([0, 0, 2, 2, 4, 3, 4, 7, 0], dtype=np.int64)


def _ped(gen, ind, fa, mo):
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)


def _founders(n):
    return np.arange(1, n + 1, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)


def test_the_oracle_on_hand_made_labels():
    """Five probands in the groups 0, 0, 1, 2, 2; four labels; two simulations.
    s = 0: (0, 0), (0, 1) | (0, 2) | (3, 3), (3, 0).          s = 1: (1, 2), (2, 2) | (2, 2) | (0, 1), (1, 1).
    Group 0 at s = 0 holds three copies of label 0, two in the first proband and one in the second: 2 x 1 = 2 matching pairs between
    different probands, (9 - 2 - 3) / 2.  Groups 0 and 1 at s = 1 hold 3 and 2 copies of label 2: 6 pairs."""
    labels = np.array([[[0, 1], [0, 2]],
                       [[0, 2], [1, 2]],
                       [[0, 2], [2, 2]],
                       [[3, 0], [3, 1]],
                       [[3, 1], [0, 1]]], dtype=np.int32)
    group = np.array([0, 0, 1, 2, 2])
    copies, autozygous, matches, by_pro = tables(labels, group, 3, 4)
    assert copies.tolist() == [[3, 2, 3, 0], [1, 0, 3, 0], [2, 3, 0, 3]]
    assert autozygous.tolist() == [[1, 0, 1, 0], [0, 0, 1, 0], [0, 1, 0, 1]]
    assert [pair_index(a, b, 3) for a in range(3) for b in range(a, 3)] == [0, 1, 2, 3, 4, 5]
    assert matches.tolist() == [[2, 0, 2, 0],          # (0, 0)
                                [3, 0, 6, 0],          # (0, 1)
                                [3, 3, 0, 0],          # (0, 2)
                                [0, 0, 0, 0],          # (1, 1): one proband, no pair
                                [1, 0, 0, 0],          # (1, 2)
                                [0, 2, 0, 2]]          # (2, 2)
    assert by_pro.tolist() == [[1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 1, 0, 0]]
    assert copies.dtype == autozygous.dtype == matches.dtype == np.int64 and by_pro.dtype == np.int32
    assert np.array_equal(matches_by_pairs(labels, group, 3, 4), matches)
    one = tables(labels, np.zeros(5, dtype=np.int64), 1, 4)
    assert one[0].tolist() == [[6, 5, 6, 3]] and one[1].tolist() == [[1, 1, 2, 1]] and one[2].tolist() == [[9, 5, 8, 2]]
    assert check_invariants(copies, autozygous, matches, by_pro, [2, 1, 2], 2, group=group, merged=one[:3]) == 0
    # merging 1 and 2, and the empty group 3 of a wider table
    c, z, m = merge(copies, autozygous, matches, 3, [[0], [1, 2]])
    want = tables(labels, np.array([0, 0, 1, 1, 1]), 2, 4)
    assert np.array_equal(c, want[0]) and np.array_equal(z, want[1]) and np.array_equal(m, want[2])
    wide = tables(labels, group, 4, 4)
    assert not wide[0][3].any() and not wide[2][[pair_index(a, 3, 4) for a in range(4)]].any() and np.array_equal(wide[0][:3], copies)
    with pytest.raises(AssertionError):
        check_invariants(copies + 1, autozygous, matches, by_pro, [2, 1, 2], 2)


def test_invariants_on_the_reference():
    """The invariants on the reference itself: 1, 4, 5, 6, 7; 2 against the reference of gen.simuCarriers; 3 against the identity states
    of tests/ident_oracle.py; the matches against the literal count over pairs of probands."""
    rng = np.random.default_rng(5)
    ind, fa, mo, _ = random_pedigree(rng, 300, p_founder=0.08, p_one_parent=0.1, p_selfing=0.05, max_back=25)
    pro = rng.choice(ind[100:], size=16, replace=False).astype(np.int64)
    pro[9], pro[13], pro[4] = pro[1], pro[1], ind[0]
    groups = np.array([-1, 2, 0, 1, 1, 0, 1, 0, -1, 2, 0, 1, 2, 2, 0, 1])             # 1, 9 and 13 are one proband; 4 is a founder
    G, S = 4, 300                                                                    # group 3 is empty
    ref = OriginVector(ind, fa, mo, pro, groups, G, S, 31)
    copies, autozygous, matches, by_pro = ref.at(S)
    assert ref.n == len(np.unique(pro[groups >= 0])) and ref.sizes[3] == 0 and ref.sizes.min(initial=9, where=ref.sizes > 0) >= 2
    one = OriginVector(ind, fa, mo, pro, np.where(groups >= 0, 0, -1), 1, S, 31)
    assert check_invariants(copies, autozygous, matches, by_pro, ref.sizes, S, ref.alleles, ref.pro, ref.group, merged=one.at(S)[:3]) >= 1
    assert autozygous.any() and matches[pair_index(0, 1, G)].any() and matches[pair_index(2, 2, G)].any()
    assert np.array_equal(matches_by_pairs(ref.labels, ref.group, G, ref.n_labels), matches)
    # 2: G = 1 against the reference of gen.simuCarriers on the same labels
    carriers, homozygotes, _ = carry_tables(one.labels, one.labels[:0], one.n_labels)
    weight = np.arange(carriers.shape[1], dtype=np.int64)
    assert np.array_equal(one.at(S)[0][0], (carriers.astype(np.int64) + homozygotes) @ weight)
    assert np.array_equal(one.at(S)[1][0], homozygotes.astype(np.int64) @ weight)
    # 3: the numerator of the kinship of the identity states, pair by pair
    c = counts_of(ref.labels).astype(np.int64)
    num = 4 * c[..., 0] + 2 * (c[..., 2] + c[..., 4] + c[..., 6]) + c[..., 7]
    for a in range(G):
        ia = np.flatnonzero(ref.group == a)
        assert autozygous[a].sum() == c[ia, ia, 0].sum()
        for b in range(a, G):
            ib = np.flatnonzero(ref.group == b)
            block = num[np.ix_(ia, ib)]
            assert matches[pair_index(a, b, G)].sum() == (np.triu(block, 1).sum() if a == b else block.sum())
    # 7: order and repeats; renumbering the groups permutes the tables
    order = rng.permutation(len(pro))
    again = OriginVector(ind, fa, mo, np.concatenate([pro[order], pro[:5]]), np.concatenate([groups[order], groups[:5]]), G, S, 31)
    back = np.array([again.pro.tolist().index(p) for p in ref.pro.tolist()])
    t = again.at(S)
    check_invariants(t[0], t[1], t[2], t[3][back], ref.sizes, S, other=ref.at(S))
    perm = np.array([2, 0, 3, 1])                                                    # old group a is new group perm[a]
    moved = OriginVector(ind, fa, mo, pro, np.where(groups >= 0, perm[groups], -1), G, S, 31).at(S)
    for a in range(G):
        assert np.array_equal(moved[0][perm[a]], copies[a]) and np.array_equal(moved[1][perm[a]], autozygous[a])
        for b in range(a, G):
            x, y = sorted((perm[a], perm[b]))
            assert np.array_equal(moved[2][pair_index(x, y, G)], matches[pair_index(a, b, G)])
    assert np.array_equal(moved[3], by_pro)
    # the exact recursions: frequencies sum to 1, a proband's kinship with itself is not a pair
    freq = expected_frequency(ref.o, ref.pro, ref.group, G)
    assert np.allclose(freq[:3].sum(axis=1), 1.0, atol=1e-12) and not freq[3].any()
    assert np.abs(copies[:3] / (2.0 * ref.sizes[:3, None] * S) - freq[:3]).max() <= 5 / np.sqrt(S)
    kin = exact_kinship(ref.o, ref.pro, ref.group, G)
    assert np.isnan(kin[3]).all() and np.nanmax(kin) <= 0.5 and np.array_equal(kin[:3, :3], kin[:3, :3].T)


def _check_plan(gen, ind, fa, mo, pro, groups, G, **kw):
    h = gen.OriginsPlan(ind, fa, mo, pro, groups, n_groups=G, simul_no=64, seed=1, **kw)
    g = gen.IdentityPlan(ind, fa, mo, np.asarray(pro, dtype=np.int64), simul_no=64, seed=1)
    try:
        assert (h.n_live, h.levels, h.n_labels, h.planes, h.n_pro) == (g.n_live, g.levels, g.n_labels, g.planes, g.n_pro)
        assert np.array_equal(h.rows_per_level(), g.rows_per_level())
        got = h.alleles()
        assert got.dtype == np.int64 and np.array_equal(got, g.alleles())
        st, gs = h.stats(), g.stats()
        assert st["sweep_ms"] == 0.0 and st["count_ms"] == 0.0 and st["count_bytes"] == 0.0
        assert (st["planes"], st["levels"], st["panel_cols"], st["panels"]) == (gs["planes"], gs["levels"], gs["panel_cols"], gs["panels"])
        keep = np.ones(len(pro), bool) if groups is None else np.asarray(groups) >= 0
        assert (st["n_groups"], st["n"]) == (G, len(np.unique(np.asarray(pro)[keep]))) == (h.n_groups, h.n_grouped)
        assert h.n_pairs == G * (G + 1) // 2
        return h.n_labels, st
    finally:
        h.close()
        g.close()


def test_plan_is_the_identity_plan_on_the_list_as_given(gen):
    ped = gen.genealogy(gen.geneaJi)
    pro = gen.pro(ped)
    n_labels, st = _check_plan(gen, ped.ind, ped.father, ped.mother, pro, None, 1)
    assert (st["chunk_labels"], st["chunks"], st["lds_bytes"]) == (n_labels, 1, 256 * (n_labels | 1))
    _check_plan(gen, ped.ind, ped.father, ped.mother, pro[[2, 0, 2]], [1, -1, 1], 2)
    rng = np.random.default_rng(99)
    seen = set()
    for k in range(60):
        ind, fa, mo, _ = random_pedigree(rng, int(rng.integers(2, 400)), p_founder=0.15, p_one_parent=0.1, p_selfing=0.03, max_back=40)
        G = [1, 2, 7, 32][k % 4]
        distinct = rng.permutation(ind)[: int(rng.integers(1, min(12, len(ind)) + 1))]
        of = dict(zip(distinct.tolist(), rng.integers(-1, G, size=len(distinct)).tolist()))
        of[int(distinct[0])] = G - 1
        pro = rng.choice(distinct, size=len(distinct) + int(rng.integers(0, 3)), replace=True).astype(np.int64)
        pro[0] = distinct[0]
        groups = np.array([of[int(p)] for p in pro.tolist()], dtype=np.int32)
        arg = [0, 1, 5, 1000][(k // 4) % 4]
        n_labels, st = _check_plan(gen, ind, fa, mo, pro, groups if k % 8 else (None if G == 1 else groups), G, chunk_labels=arg, by_proband=bool(k % 2))
        lc = min(n_labels, 639 // G, arg if arg else 639 // G)
        assert (st["chunk_labels"], st["chunks"], st["lds_bytes"]) == (lc, -(-n_labels // lc), 256 * ((lc * G) | 1))
        assert st["lds_bytes"] <= 163840
        seen.add(st["chunks"])
    assert len(seen) >= 3


def test_planned_shapes(gen):
    h = gen.OriginsPlan(IND, FA, MO, [8, 6, 8, 9], [1, 0, 1, -1], n_groups=3, simul_no=5000, seed=3, panel_cols=1000, chunk_labels=2, by_proband=True)
    try:
        assert (h.n_live, h.levels, h.n_labels, h.planes, h.n_pro, h.simul_no, h.seed) == (9, 4, 7, 3, 4, 5000, 3)
        assert h.alleles().tolist() == [[1, 0], [1, 1], [2, 0], [2, 1], [7, 0], [9, 0], [9, 1]]
        assert (h.n_groups, h.n_grouped, h.n_pairs, h.by_proband) == (3, 2, 6, True)
        st = h.stats()
        assert (st["panel_cols"], st["panels"], st["chunk_labels"], st["chunks"], st["lds_bytes"]) == (1024, 5, 2, 4, 256 * 7)
    finally:
        h.close()


def test_argument_errors(gen):
    ok = dict(pro_ids=[8, 6], groups=[0, 1], n_groups=2, simul_no=10, seed=3)

    def plan(**kw):
        a = {**ok, **kw}
        gen.OriginsPlan(a.pop("ind", IND), a.pop("fa", FA), a.pop("mo", MO), **a).close()

    plan()
    plan(groups=None, n_groups=1)
    plan(simul_no=1 << 24)
    plan(simul_no=1, panel_cols=7, chunk_labels=7, by_proband=True)
    plan(chunk_labels=2**31 - 1)
    plan(pro_ids=[8, 8, 6, 9], groups=[1, 1, 0, -1])
    plan(pro_ids=[8, 6, 9, 9], groups=[0, -1, -1, -1], n_groups=32)
    with pytest.raises(KeyError):
        plan(pro_ids=[8, 99])
    with pytest.raises(KeyError):
        plan(pro_ids=[0, 8])
    for kw in (dict(simul_no=0), dict(simul_no=-5), dict(simul_no=(1 << 24) + 1), dict(pro_ids=[], groups=[]), dict(panel_cols=-1), dict(chunk_labels=-1),
               dict(n_groups=0), dict(n_groups=33), dict(n_groups=-1), dict(groups=None, n_groups=2), dict(groups=[0, 2]), dict(groups=[-2, 0]),
               dict(groups=[0]), dict(groups=[0, 1, 1]), dict(groups=[0.5, 1]), dict(groups=[-1, -1])):
        with pytest.raises(ValueError):
            plan(**kw)
    for pro, groups in (([8, 6, 8], [0, 1, 1]), ([8, 8], [0, -1]), ([8, 6, 9, 6], [-1, 1, 0, -1])):
        with pytest.raises(ValueError, match="two different groups"):
            plan(pro_ids=pro, groups=groups)
    with pytest.raises(ValueError, match="no listed proband is in a group"):
        plan(groups=[-1, -1])
    with pytest.raises(Exception, match="duplicate"):
        plan(ind=np.array([1, 2, 3, 4, 5, 6, 7, 8, 1]))
    with pytest.raises(Exception, match="rank order"):
        plan(fa=np.array([8, 0, 1, 1, 3, 3, 0, 5, 0]))
    # the C entry point itself: NULL out, NULL lists, negative sizes, a by_proband that is no flag, NULL handles
    L = gen._capi.lib()
    i64, i32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    pro, grp = np.array([8], dtype=np.int64), np.array([0], dtype=np.int32)
    ped = [len(IND), IND.ctypes.data_as(i64), FA.ctypes.data_as(i64), MO.ctypes.data_as(i64)]
    h = ctypes.c_void_p()
    ARG = gen._capi.GENPHI_ERR_ARG
    assert L.genphi_origin_create(*ped, 1, pro.ctypes.data_as(i64), grp.ctypes.data_as(i32), 1, 10, 3, 0, 0, 0, None) == ARG
    assert L.genphi_origin_create(*ped, 1, None, None, 1, 10, 3, 0, 0, 0, ctypes.byref(h)) == ARG and not h.value
    assert L.genphi_origin_create(*ped, -1, pro.ctypes.data_as(i64), None, 1, 10, 3, 0, 0, 0, ctypes.byref(h)) == ARG and not h.value
    assert L.genphi_origin_create(*ped, 0, pro.ctypes.data_as(i64), None, 1, 10, 3, 0, 0, 0, ctypes.byref(h)) == ARG and not h.value
    assert L.genphi_origin_create(*ped, 1, pro.ctypes.data_as(i64), None, 1, 10, 3, 0, 0, 2, ctypes.byref(h)) == ARG and not h.value
    assert L.genphi_origin_create(*ped, 1, pro.ctypes.data_as(i64), None, 1, 10, 3, 0, 0, -1, ctypes.byref(h)) == ARG and not h.value
    assert L.genphi_origin_create(ped[0], None, ped[2], ped[3], 1, pro.ctypes.data_as(i64), None, 1, 10, 3, 0, 0, 0, ctypes.byref(h)) == ARG and not h.value
    assert L.genphi_origin_create(*ped, 1, pro.ctypes.data_as(i64), None, 1, 10, 3, 0, 0, 0, ctypes.byref(h)) == 0 and h.value
    assert L.genphi_origin_by_proband_to_host(h, None) == ARG                          # not requested
    L.genphi_origin_destroy(h)
    assert L.genphi_origin_levels(None, None, None, None) == ARG and L.genphi_origin_alleles(None, None, None, None, None) == ARG
    assert L.genphi_origin_compute(None, 0) == ARG
    assert L.genphi_origin_stats(None, *([None] * 13)) == ARG
    for name in ("copies", "autozygous", "matches", "by_proband"):
        assert getattr(L, "genphi_origin_%s_to_host" % name)(None, None) == ARG
    L.genphi_origin_destroy(None)
    hp = gen.OriginsPlan(IND, FA, MO, [8, 6], simul_no=10, seed=3, by_proband=True)
    for fn in (hp.copies_to_host, hp.autozygous_to_host, hp.matches_to_host, hp.by_proband_to_host):
        with pytest.raises(ValueError, match="nothing computed"):
            fn()
    hp.close()
    hp = gen.OriginsPlan(IND, FA, MO, [8, 6], simul_no=10, seed=3)
    with pytest.raises(ValueError, match="without by_proband"):
        hp.by_proband_to_host()
    hp.close()
    ped = _ped(gen, IND, FA, MO)
    with pytest.raises(ValueError):
        gen.simuOrigins(ped, pro=[])
    with pytest.raises(KeyError):
        gen.simuOrigins(ped, pro=[77])
    with pytest.raises(ValueError):
        gen.simuOrigins(ped, pro=[8, 6], groups={})
    with pytest.raises(ValueError):
        gen.simuOrigins(ped, pro=[8, 6], groups={5: "a"})                              # nobody listed is in a group
    with pytest.raises(ValueError):
        gen.simuOrigins(ped, pro=[8, 6], groups={k: "g%d" % k for k in range(1, 34)})  # 33 names
    with pytest.raises(ValueError):
        gen.simuOrigins(ped, simulNo=0)
    with pytest.raises(TypeError):
        gen.simuOrigins(ped, controls=[1])
    h1, h2 = gen.OriginsPlan(IND, FA, MO, [8]), gen.OriginsPlan(IND, FA, MO, [8])
    assert 0 <= h1.seed < 2**64 and h1.seed != h2.seed and h1.simul_no == 5000
    h1.close()
    h2.close()


def test_the_limits_on_unrelated_founders(gen):
    """32,767 distinct probands in a group are taken and 32,768 refused; repeats and ungrouped probands do not count.  32,768 founders
    have 65,536 labels: by proband that is 2^31 cells, one too many."""
    ind, fa, mo = _founders(32780)
    h = gen.OriginsPlan(ind, fa, mo, ind[:32767], simul_no=64, seed=1, by_proband=True)
    try:
        assert (h.n_grouped, h.n_labels, h.planes) == (32767, 65534, 16) and h.n_grouped * h.n_labels < 2**31
        st = h.stats()
        assert (st["chunk_labels"], st["chunks"], st["lds_bytes"]) == (639, 103, 163584)                # the default chunk is the widest
    finally:
        h.close()
    groups = np.concatenate([np.zeros(32767, dtype=np.int32), np.full(5, -1, dtype=np.int32), np.zeros(40, dtype=np.int32)])
    gen.OriginsPlan(ind, fa, mo, np.concatenate([ind[:32772], ind[:40]]), groups, simul_no=64, seed=1).close()
    with pytest.raises(ValueError, match="32,767"):
        gen.OriginsPlan(ind, fa, mo, ind[:32768], simul_no=64, seed=1)
    two = np.concatenate([np.zeros(32767, dtype=np.int32), np.ones(1, dtype=np.int32)])
    h = gen.OriginsPlan(ind, fa, mo, ind[:32768], two, n_groups=2, simul_no=64, seed=1)
    try:
        assert (h.n_grouped, h.n_labels) == (32768, 65536)
        assert (h.stats()["chunk_labels"], h.stats()["chunks"]) == (319, 206)
    finally:
        h.close()
    with pytest.raises(ValueError, match="cells"):
        gen.OriginsPlan(ind, fa, mo, ind[:32768], two, n_groups=2, simul_no=64, seed=1, by_proband=True)
    with pytest.raises(ValueError, match="32,767"):
        gen.OriginsPlan(ind, fa, mo, ind[:32770], np.concatenate([two[::-1], [0, 1]]), n_groups=2, simul_no=64, seed=1)


def test_symbols_are_exported_declared_and_bound(gen):
    from genlib_jl_amd import _capi
    header = open(os.path.join(ROOT, "include", "genphi.h")).read()
    L = ctypes.CDLL(_capi.LIB_PATH)
    names = ["genphi_origin_" + n for n in ("create", "levels", "alleles", "compute", "copies_to_host", "autozygous_to_host", "matches_to_host",
                                            "by_proband_to_host", "stats", "destroy")]
    for name in names:
        assert hasattr(L, name) and name in _capi.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, header), name
    assert sum(n.startswith("genphi_origin_") for n in _capi.EXPORTED_SYMBOLS) == 10
    assert len(_capi.lib().genphi_origin_create.argtypes) == 14 and len(_capi.lib().genphi_origin_stats.argtypes) == 14
    assert gen.OriginsPlan is _capi.OriginsPlan and issubclass(gen.OriginsPlan, _capi._SweepPlan) and gen.simuOrigins.__doc__ and gen.SimuOrigins.__doc__
    text = header[header.index("gen.simuOrigins"):header.index("typedef struct genphi_origin")]
    for k in range(1, 8):
        assert re.search(r"^ \*\s+%d\. " % k, text, re.M), k
    for word in ("copies[a, l]", "autozygous[a, l]", "matches[p, l]", "autozygous_pro[i, l]", "32,767", "Not offered"):
        assert word in text, word
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"origin.hip"' in entry and '"origin.h"' in entry


def test_SimuOrigins_shares(gen):
    """The shares from hand-made integer tables, S = 10: groups a (two probands) and b (one), founder 10 (two alleles) and
    half-founder 20."""
    alleles = np.array([[10, 0], [10, 1], [20, 1]], dtype=np.int64)
    copies = np.array([[20, 12, 8], [10, 0, 10]], dtype=np.int64)
    autozygous = np.array([[2, 0, 1], [1, 0, 0]], dtype=np.int64)
    matches = np.zeros((2, 2, 3), dtype=np.int64)
    matches[0, 0] = [4, 2, 2]
    matches[0, 1] = matches[1, 0] = [6, 0, 10]
    by_pro = np.array([[2, 0, 0], [0, 0, 1], [1, 0, 0]], dtype=np.int32)
    r = gen.SimuOrigins(np.array([7, 8, 9]), alleles, ["a", "b"], [2, 1], copies, autozygous, matches, by_pro, 10, 1)
    assert r.founders.tolist() == [10, 20] and r.sizes.tolist() == [2, 1] and r.names == ["a", "b"]
    assert r.frequency.dtype == np.float64 and r.frequency.tolist() == [[20 / 40, 12 / 40, 8 / 40], [10 / 20, 0.0, 10 / 20]]
    kin = r.kinship
    assert kin[0, 0] == 8 / 40 and kin[0, 1] == kin[1, 0] == 16 / 80 and np.isnan(kin[1, 1])
    by = r.kinship_by_allele
    assert by[0, 0].tolist() == [4 / 40, 2 / 40, 2 / 40] and by[0, 1].tolist() == by[1, 0].tolist() == [6 / 80, 0.0, 10 / 80] and np.isnan(by[1, 1]).all()
    byf = r.kinship_by_founder()
    assert byf.shape == (2, 2, 2) and byf[0, 0].tolist() == [6 / 40, 2 / 40] and byf[1, 0].tolist() == [6 / 80, 10 / 80]
    assert r.share[0, 0].tolist() == [4 / 8, 2 / 8, 2 / 8] and r.share[0, 1].tolist() == [6 / 16, 0.0, 10 / 16] and r.share[1, 1].tolist() == [0.0] * 3
    assert r.inbreeding.tolist() == [3 / 20, 1 / 10]
    assert r.inbreeding_by_founder().tolist() == [[2 / 20, 1 / 20], [1 / 10, 0.0]]
    assert r.partial_inbreeding().tolist() == [[2 / 10, 0.0], [0.0, 1 / 10], [1 / 10, 0.0]]
    assert r.ranking("a", "a").tolist() == [0, 1, 2] and r.ranking("a", "b").tolist() == [2, 0, 1] and r.ranking("b", "a", k=1).tolist() == [2]
    assert r.ranking("b", "b").tolist() == [0, 1, 2] and r.ranking("a", "b", k=0).tolist() == []
    with pytest.raises(KeyError):
        r.ranking("a", "c")
    assert "3 probands in 2 groups" in repr(r) and "3 founder alleles" in repr(r)
    none = gen.SimuOrigins(np.array([7, 8, 9]), alleles, ["a", "b"], [2, 1], copies, autozygous, matches, None, 10, 1)
    with pytest.raises(ValueError):
        none.partial_inbreeding()
    empty = gen.SimuOrigins(np.array([7, 8]), alleles, ["a", "b"], [2, 0], copies * [[1], [0]], autozygous * [[1], [0]], matches * 0, None, 10, 1)
    assert np.isnan(empty.frequency[1]).all() and np.isnan(empty.inbreeding[1]) and empty.kinship[0, 0] == 0.0 and np.isnan(empty.kinship[0, 1])


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_origin_h_as_a_stand_alone_program(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "origin_check")
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra"] + flags + [os.path.join(ROOT, "tests", "origin_check.cpp"), "-o", exe]
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
    cases, walked, plans, conflicts, ranges, repeats, ungrouped, violations = (int(v) for v in m.groups())
    assert violations == 0 and cases >= 3000 and walked > 10**7 and plans == 20000 and conflicts > 1000 and ranges > 500 and repeats > 1000 and ungrouped > 1000
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
