"""gen.simuSharing without a GPU: genphi_link_words (the host restatement of what the step kernel draws, csrc/link.cpp) against the
reference of tests/link_oracle.py, the properties of the crossover and transmission words, the share of set crossover bits, the host
plan of gen.SharingPlan against gen.IdentityPlan's, every argument error, the invariants of the definition (include/genphi.h) on the
reference itself, the shares of gen.SimuSharing from hand-made sums, and the host code as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/link_check.cpp, which also adds up link_sizes)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from link_oracle import LinkVector, bits_of, crossover_words, sums_of, transmission, words_of
from random_pedigree import random_pedigree
from simu_oracle import philox_vector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genlib.jl_amd", "csrc")
DATA = os.path.join(ROOT, "genlib.jl_amd", "data")

SUMMARY = re.compile(r"^link check: (\d+) cases, (\d+) loci, (\d+) crossovers, (\d+) refusals, (\d+) plans; (\d+) violations$", re.M)

LOCI = [1, 63, 64, 65, 128, 129, 4096]
QS = [0, 1, 64, 0x5555, 32767, 32768]


def _args(ped):
    return ped.ind, ped.father, ped.mother


def shapes_pedigree():
    """1, 2 founders; 3 = (1, 2); 4 = (1, 2); 5 = (3, 4) inbred; 6 = (3, 3) selfed; 7 = (0, 4) half-founder; 8 = (5, 7); 9 founder."""
    ind = np.arange(1, 10, dtype=np.int64)
    fa = np.array([0, 0, 1, 1, 3, 3, 0, 5, 0], dtype=np.int64)
    mo = np.array([0, 0, 2, 2, 4, 3, 4, 7, 0], dtype=np.int64)
    return ind, fa, mo


@pytest.mark.parametrize("L", LOCI)
def test_words_match_the_oracle(gen, L):
    W = (L + 63) // 64
    for q in QS:
        for seed, ID, side, s in ((77, 12345678901, 1, 5), (2**64 - 1, 3, 0, 2**24 - 1), (0, -4, 1, 0)):
            X, T = gen._capi.link_words(seed, ID, side, s, L, q)
            assert X.dtype == np.uint64 and X.shape == T.shape == (W,)
            want = crossover_words([ID], side, [s], W, q, seed)[0, 0]
            assert np.array_equal(X, want), (L, q, seed)
            want_T = transmission(want, L)
            assert np.array_equal(bits_of(T, L).astype(bool), want_T), (L, q, seed)
            # the bits of T past L, in the last word, run on as if the chromosome did: X is drawn by whole words
            assert np.array_equal(T, words_of((np.cumsum(bits_of(X, 64 * W), dtype=np.int64) & 1).astype(np.uint8)))


def test_no_recombination_gives_a_constant_transmission_word(gen):
    seen = set()
    for s in range(64):
        X, T = gen._capi.link_words(5, 1001, 0, s, 4096, 0)
        assert np.all(X[1:] == 0) and X[0] in (0, 1)
        assert np.all(T == (np.uint64(0xFFFFFFFFFFFFFFFF) if X[0] else np.uint64(0)))
        seen.add(int(X[0]))
    assert seen == {0, 1}                                                            # the starting strand is a coin


def test_independent_loci_take_the_last_word_of_the_fold(gen):
    """q = 32768 has bit 15 alone: X = U_15, the second word of block 7, apart from bit 0 of word 0."""
    seed, ID, side, s, W = 99, 7 + (5 << 32), 1, 123456, 64
    X, _ = gen._capi.link_words(seed, ID, side, s, 4096, 32768)
    w = np.arange(W, dtype=np.uint64)
    _, _, o2, o3 = philox_vector(ID & 0xFFFFFFFF, ID >> 32, s, np.uint64(0x80000000 | side | 7 << 8) | (w << np.uint64(1)), seed & 0xFFFFFFFF, seed >> 32)
    U15 = o2 | (o3 << np.uint64(32))
    assert np.array_equal(X[1:], U15[1:]) and (X[0] ^ U15[0]) in (0, 1)
    o0 = philox_vector(ID & 0xFFFFFFFF, ID >> 32, s, 0x80000000 | side | 8 << 8, seed & 0xFFFFFFFF, seed >> 32)[0]
    assert int(X[0]) & 1 == int(o0) & 1


def test_words_change_with_side_simulation_word_and_ID(gen):
    base = dict(seed=11, ID=40, side=0, s=9)

    def draw(q, **kw):
        a = {**base, **kw}
        return np.stack([gen._capi.link_words(a["seed"], a["ID"], a["side"], s, 256, q)[0] for s in range(a["s"], a["s"] + 64)])

    X = draw(0x5555)
    for kw in (dict(side=1), dict(s=9 + 64), dict(ID=41), dict(ID=40 + (1 << 32)), dict(seed=12), dict(seed=11 + (1 << 32))):
        Y = draw(0x5555, **kw)
        assert np.all(X[:, 1:] != Y[:, 1:])                                          # 64-bit words at r = 1/3: never equal by chance
        assert 8 <= int(((X[:, 0] ^ Y[:, 0]) & np.uint64(1)).sum()) <= 56            # the start bits: 64 fair coins, 6 sigma
    assert len(np.unique(X)) == X.size                                               # every word and simulation draws its own
    S0 = draw(0)[:, 0]
    for kw in (dict(side=1), dict(s=9 + 64), dict(ID=41), dict(seed=12)):
        assert 8 <= int((S0 ^ draw(0, **kw)[:, 0]).sum()) <= 56


@pytest.mark.parametrize("q", [64, 0x5555])
def test_share_of_set_crossover_bits(gen, q):
    """2^20 intervals between neighbouring loci (257 chromosomes of 4096 loci under seed 2027, the starting bit left out, cut to 2^20):
    the share of crossovers lies within 6 sqrt(r (1 - r) / n) of r = q / 65536."""
    n, r = 1 << 20, q / 65536.0
    bits = np.concatenate([bits_of(gen._capi.link_words(2027, 600 + (s & 1), s & 1, s, 4096, q)[0], 4096)[1:] for s in range(257)])[:n]
    assert len(bits) == n
    share = bits.mean(dtype=np.float64)
    print("q = %d: %d crossovers in 2^20 intervals, share %.6f against r = %.6f (%.2f sigma)" % (q, bits.sum(), share, r, (share - r) / np.sqrt(r * (1 - r) / n)))
    assert abs(share - r) <= 6.0 * np.sqrt(r * (1.0 - r) / n)


def _same_plan(gen, ind, fa, mo, pro):
    a = gen.SharingPlan(ind, fa, mo, pro, loci=130, q=64, simul_no=7, seed=1)
    b = gen.IdentityPlan(ind, fa, mo, pro, simul_no=7, seed=1)
    try:
        assert (a.n_live, a.levels, a.n_labels, a.planes, a.n_pro) == (b.n_live, b.levels, b.n_labels, b.planes, b.n_pro)
        assert np.array_equal(a.rows_per_level(), b.rows_per_level()) and np.array_equal(a.alleles(), b.alleles())
        st = a.stats()
        assert st["sweep_ms"] == 0.0 and st["pair_ms"] == 0.0 and st["planes"] == b.planes and st["levels"] == b.levels
        assert (st["tile_rows"], st["tile_cols"], st["panel_sims"], st["panels"], st["lanes_per_sim"]) == (32, 32, 7, 1, 2)
        return a.n_live
    finally:
        a.close()
        b.close()


def test_plan_is_ident_s(gen):
    for name in ("geneaJi.csv", "genea140.csv"):
        ped = gen.genealogy(os.path.join(DATA, name))
        _same_plan(gen, *_args(ped), gen.pro(ped))
        _same_plan(gen, *_args(ped), gen.pro(ped)[[2, 0, 2]])
        _same_plan(gen, *_args(ped), ped.ind[:1])
    rng = np.random.default_rng(2)
    live = 0
    for _ in range(60):
        ind, fa, mo, _ = random_pedigree(rng, int(rng.integers(1, 300)), p_founder=0.15, p_one_parent=0.1, p_selfing=0.03, max_back=40)
        live += _same_plan(gen, ind, fa, mo, rng.choice(ind, size=int(rng.integers(1, 10)), replace=True).astype(np.int64))
    assert live > 300


def test_planned_shapes(gen):
    ind, fa, mo = shapes_pedigree()
    for L, lanes in ((1, 1), (128, 1), (129, 2), (256, 2), (257, 4), (1024, 8), (1025, 16), (2048, 16), (2049, 32), (4096, 32)):
        h = gen.SharingPlan(ind, fa, mo, [8, 6, 8], loci=L, q=0, simul_no=5000, seed=3, panel_sims=1000)
        st = h.stats()
        assert (st["panel_sims"], st["panels"], st["lanes_per_sim"]) == (1000, 5, lanes) and (h.loci, h.q, h.simul_no, h.seed) == (L, 0, 5000, 3)
        h.close()
    h = gen.SharingPlan(ind, fa, mo, [8, 6, 8], simul_no=10, panel_sims=3)
    assert (h.loci, h.q, h.n_live, h.levels, h.n_labels, h.planes, h.n_pro) == (1024, 64, 8, 4, 5, 3, 3) and h.stats()["panels"] == 4
    h.close()


def test_argument_errors(gen):
    ind, fa, mo = shapes_pedigree()
    ok = dict(pro_ids=[8, 6], loci=100, q=64, simul_no=10, seed=3)

    def plan(**kw):
        a = {**ok, **kw}
        gen.SharingPlan(a.pop("ind", ind), a.pop("fa", fa), a.pop("mo", mo), **a).close()

    plan()
    for kw in (dict(simul_no=1 << 24), dict(loci=1), dict(loci=4096), dict(q=0), dict(q=32768), dict(simul_no=1, labels=True, all_pairs=True, panel_sims=7),
               dict(pro_ids=[8] * 46340)):
        plan(**kw)
    with pytest.raises(KeyError):
        plan(pro_ids=[8, 99])
    with pytest.raises(KeyError):
        plan(pro_ids=[0])
    for kw in (dict(simul_no=0), dict(simul_no=-5), dict(simul_no=(1 << 24) + 1), dict(pro_ids=[]), dict(pro_ids=[8] * 46341), dict(panel_sims=-1),
               dict(loci=0), dict(loci=-1), dict(loci=4097), dict(loci=1 << 40), dict(q=-1), dict(q=32769), dict(q=65536)):
        with pytest.raises(ValueError):
            plan(**kw)
    with pytest.raises(MemoryError):
        plan(pro_ids=[8] * 4096, loci=4096, simul_no=1 << 24, labels=True)               # 2^51 bytes of labels
    with pytest.raises(Exception, match="duplicate"):
        plan(ind=np.array([1, 2, 3, 4, 5, 6, 7, 8, 1]))
    with pytest.raises(Exception, match="rank order"):
        plan(fa=np.array([8, 0, 1, 1, 3, 3, 0, 5, 0]))
    # the C entry points themselves: NULL out, an unknown flag, NULL handles
    L = gen._capi.lib()
    i64 = ctypes.POINTER(ctypes.c_int64)
    pro = np.array([8], dtype=np.int64)
    a = [len(ind), ind.ctypes.data_as(i64), fa.ctypes.data_as(i64), mo.ctypes.data_as(i64), 1, pro.ctypes.data_as(i64), 100, 64, 10, 3, 0]
    h = ctypes.c_void_p()
    ARG = gen._capi.GENPHI_ERR_ARG
    assert L.genphi_link_create(*a, 4, ctypes.byref(h)) == ARG and not h.value
    assert L.genphi_link_create(*a, 0, None) == ARG
    assert L.genphi_link_levels(None, None, None, None) == ARG and L.genphi_link_alleles(None, None, None, None, None) == ARG
    assert L.genphi_link_sums_to_host(None, None) == ARG and L.genphi_link_labels_to_host(None, None) == ARG
    assert L.genphi_link_stats(None, *[None] * 12) == ARG and L.genphi_link_compute(None, 0) == ARG
    L.genphi_link_destroy(None)
    # nothing computed yet; labels without the flag
    hp = gen.SharingPlan(ind, fa, mo, [8, 6], simul_no=10, seed=3)
    with pytest.raises(ValueError, match="nothing computed"):
        hp.sums_to_host()
    with pytest.raises(ValueError, match="GENPHI_LINK_FLAG_LABELS"):
        hp.labels_to_host()
    hp.close()
    hp = gen.SharingPlan(ind, fa, mo, [8, 6], simul_no=10, seed=3, labels=True)
    with pytest.raises(ValueError, match="nothing computed"):
        hp.labels_to_host()
    hp.close()
    for bad in (dict(loci=0), dict(loci=4097), dict(q=-1), dict(q=32769), dict(side=2), dict(side=-1), dict(s=-1), dict(s=1 << 24)):
        with pytest.raises(ValueError):
            gen._capi.link_words(**{**dict(seed=1, ID=1, side=0, s=0, loci=64, q=64), **bad})
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(9, dtype=np.int64)}, sort=False)
    for kw in (dict(pro=[]), dict(simulNo=0), dict(loci=0), dict(loci=4097), dict(probRecomb=0.51), dict(probRecomb=-0.1), dict(probRecomb=float("nan")),
               dict(length=-1.0), dict(length=float("nan"))):
        with pytest.raises(ValueError):
            gen.simuSharing(ped, **kw)
    with pytest.raises(KeyError):
        gen.simuSharing(ped, pro=[77])
    h1, h2 = gen.SharingPlan(ind, fa, mo, [8]), gen.SharingPlan(ind, fa, mo, [8])
    assert 0 <= h1.seed < 2**64 and h1.seed != h2.seed and h1.simul_no == 1000
    h1.close()
    h2.close()


def test_sharing_q(gen):
    """Haldane's map over L - 1 equal intervals, rounded to q / 65536; a given probRecomb rounded the same way."""
    assert gen.sharing_q(1024, 1.0) == round(65536 * 0.5 * (1 - np.exp(-2.0 / 1023))) == 64
    assert gen.sharing_q(2, 1e9) == 32768 and gen.sharing_q(1, 5.0) == 0 and gen.sharing_q(4096, 0.0) == 0
    assert gen.sharing_q(10, probRecomb=0.5) == 32768 and gen.sharing_q(10, probRecomb=0.0) == 0 and gen.sharing_q(10, 3.0, probRecomb=1 / 65536) == 1
    assert gen.sharing_q(10, probRecomb=0.0000076) == 0 and gen.sharing_q(10, probRecomb=0.0000077) == 1


def test_symbols_are_exported_declared_and_bound(gen):
    from genlib_jl_amd import _capi
    header = open(os.path.join(ROOT, "include", "genphi.h")).read()
    L = ctypes.CDLL(_capi.LIB_PATH)
    names = ["genphi_link_" + n for n in ("create", "levels", "alleles", "compute", "sums_to_host", "labels_to_host", "stats", "destroy", "words")]
    for name in names:
        assert hasattr(L, name) and name in _capi.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, header), name
    assert sum(n.startswith("genphi_link_") for n in _capi.EXPORTED_SYMBOLS) == 9
    assert len(_capi.lib().genphi_link_create.argtypes) == 13 and len(_capi.lib().genphi_link_stats.argtypes) == 13
    assert len(_capi.lib().genphi_link_words.argtypes) == 8
    for macro, value in (("GENPHI_LINK_FLAG_LABELS", 1), ("GENPHI_LINK_FLAG_ALL_PAIRS", 2), ("GENPHI_LINK_MAX_LOCI", 4096), ("GENPHI_LINK_MAX_Q", 32768)):
        assert re.search(r"#define %s %d\b" % (macro, value), header) and getattr(_capi, macro) == value
    assert gen.SharingPlan is _capi.SharingPlan and gen.simuSharing.__doc__ and gen.SimuSharing.__doc__


def test_SimuSharing_properties(gen):
    """The shares from hand-made sums: every one is formed once from the exact integers."""
    S, L = 10, 8
    sums = np.zeros((2, 2, 6), dtype=np.int64)
    sums[0, 0] = [2 * S * L + 40, S * 20 * 20, S * L, S * L, S, S]                    # inbred at 4 of the 8 loci of every simulation
    sums[1, 1] = [2 * S * L, S * (2 * L) ** 2, S * L, S * L, S, S]
    sums[0, 1] = sums[1, 0] = [60, 5 * 12 * 12, 48, 12, 6, 5]                         # m_s = 12 in five simulations, 0 in the others
    r = gen.SimuSharing(np.array([5, 6]), sums, L, 64, S, 1, np.zeros((2, 2), dtype=np.int64), None)
    assert r.probRecomb == 64 / 65536 and r.kinship.dtype == np.float64
    assert r.kinship.tolist() == [[200 / 320, 60 / 320], [60 / 320, 0.5]] and r.inbreeding.tolist() == [0.25, 0.0]
    assert r.ibd1[0, 1] == 48 / 80 and r.ibd2[0, 1] == 12 / 80 and r.segments[0, 1] == 0.6 and r.segment_loci[0, 1] == 8.0 and r.shared[0, 1] == 0.5
    # m_s / (4 L) is 12 / 32 in half of the simulations and 0 in the others: the standard deviation is 6 / 32
    assert r.kinship_sd[0, 1] == 6 / 32 and r.kinship_sd[1, 1] == 0.0
    assert r.labels is None and "2 probands" in repr(r)
    sums[0, 1, 2:] = 0
    assert np.isnan(gen.SimuSharing(np.array([5, 6]), sums, L, 64, S, 1, None, None).segment_loci[0, 1])
    # sums past 2^63 / S take the exact path on Python integers: S = 2^24 simulations of m_s = 2^14 each, and one of 0
    S = 1 << 24
    big = np.array([[[(S - 1) << 14, (S - 1) << 28, 0, 0, 0, 0]]], dtype=np.int64)
    sd = gen.SimuSharing(np.array([5]), big, 4096, 64, S, 1, None, None).kinship_sd[0, 0]
    assert sd == np.sqrt(float(S - 1)) / S                                           # sqrt(p (1 - p)) with p = 1 / S


@pytest.fixture(scope="module")
def mixed():
    """200 individuals with half-founders and selfing; 12 probands, two of them repeats, one a founder; labels at S = 100, L = 130."""
    rng = np.random.default_rng(5)
    ind, fa, mo, _ = random_pedigree(rng, 200, p_founder=0.08, p_one_parent=0.1, p_selfing=0.05, max_back=25)
    pro = rng.choice(ind[60:], size=12, replace=False).astype(np.int64)
    pro[9], pro[11], pro[4] = pro[1], pro[1], ind[0]
    o = LinkVector(ind, fa, mo, pro)
    return ind, fa, mo, pro, o, o.labels(100, 130, 700, 31)


def test_invariants_on_the_reference(gen, mixed):
    ind, fa, mo, pro, o, labels = mixed
    S, L = 100, 130
    s = sums_of(labels)
    assert s.dtype == np.int64 and s.shape == (12, 12, 6) and s.min() >= 0 and np.array_equal(s, s.transpose(1, 0, 2))
    k = np.arange(12)
    assert np.all(s[k, k, 2] == S * L) and np.all(s[k, k, 4] == S) and np.all(s[k, k, 5] == S)     # a diagonal pair: n1 = L and g = 1
    assert np.array_equal(s[9], s[1]) and np.array_equal(s[11], s[1])                             # repeats of one ID
    assert np.all(s[..., 3] <= s[..., 2]) and np.all(s[..., 5] <= s[..., 4]) and np.all(s[..., 4] <= s[..., 2]) and np.all(s[..., 2] <= s[..., 0])
    assert np.any(s[..., 4] > s[..., 5])                                                          # sharing in more than one segment
    # the labels of S = 3 are the first three simulations of S = 100; another seed gives other labels
    assert np.array_equal(o.labels(3, L, 700, 31), labels[:, :, :3]) and not np.array_equal(o.labels(3, L, 700, 32), labels[:, :, :3])
    # q = 0: every locus of a simulation carries the same label; g = [n1 > 0]
    flat = o.labels(20, L, 0, 31)
    s0 = sums_of(flat)
    assert np.all(flat == flat[..., :1]) and np.array_equal(s0[..., 4], s0[..., 5]) and np.all(s0[..., 0] % L == 0)
    # a sub-list of probands gives the sub-block; gen.branching first changes nothing
    sub = np.array([11, 2, 2, 7])
    assert np.array_equal(sums_of(LinkVector(ind, fa, mo, pro[sub]).labels(S, L, 700, 31)), s[np.ix_(sub, sub)])
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)
    pruned = gen.branching(ped, pro=pro)
    assert len(pruned) == o.n_live < len(ped)
    assert np.array_equal(LinkVector(pruned.ind, pruned.father, pruned.mother, pro).labels(S, L, 700, 31), labels)


def test_one_locus_is_gene_dropping_with_a_fair_coin():
    """L = 1: the only bit of T is the starting strand, so a side comes from the parent's paternal copy in about half of the
    simulations, whatever q."""
    ind, fa, mo = shapes_pedigree()
    for q in (0, 64, 32768):
        lab = LinkVector(ind, fa, mo, [3]).labels(4000, 1, q, 8)                      # 3 = (1, 2): labels 0 / 1 from 1, 2 / 3 from 2
        assert abs((lab[0, 0, :, 0] == 0).mean() - 0.5) < 0.05 and abs((lab[0, 1, :, 0] == 2).mean() - 0.5) < 0.05
        assert set(lab[0, 0].ravel().tolist()) == {0, 1} and set(lab[0, 1].ravel().tolist()) == {2, 3}


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_host_code_as_a_stand_alone_program(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "link_check")
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra", "-pthread"] + flags + [os.path.join(ROOT, "tests", "link_check.cpp"), os.path.join(CSRC, "link.cpp"),
                                                                       os.path.join(CSRC, "ident.cpp"), os.path.join(CSRC, "ancestor_sweep.cpp"),
                                                                       os.path.join(CSRC, "pedigree_index.cpp"), os.path.join(CSRC, "planner.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if san is not None and build.returncode != 0 and ("cannot find" in build.stderr or "unrecognized" in build.stderr):
        pytest.skip("this toolchain has no -fsanitize=" + san)
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("GENPHI_ENV_HOOKS", None)
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    if san is not None and run.returncode != 0 and not run.stdout and any(
            t in run.stderr for t in ("unexpected memory mapping", "runtime does not come first", "failed to intercept", "ReserveShadowMemoryRange failed")):
        pytest.skip("the sanitizer runtime does not start in this environment: " + run.stderr[:200])
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    m = SUMMARY.search(run.stdout)
    assert m, run.stdout[-1500:]
    cases, loci, crossovers, refusals, plans, violations = (int(v) for v in m.groups())
    assert violations == 0 and cases == 480 and loci > 300_000 and crossovers > 10_000 and refusals == 8 and plans == 300
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
