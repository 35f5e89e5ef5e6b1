"""gen.simuSegments without a GPU: the numpy reference of tests/segments_oracle.py against the sums of tests/link_oracle.py,
genphi_seg_host (the walk that the segment kernel runs, csrc/link_segments.h) against that reference on chromosomes given as bits,
every argument error of genphi_seg_request, the symbols, the properties of gen.SimuSegments from hand-made integers, and the host
code as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (tests/segments_check.cpp)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from link_oracle import LinkVector, sums_of, words_of
from random_pedigree import random_pedigree
from segments_oracle import reduce_bits, run_classes, segments_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genlib.jl_amd", "csrc")

SUMMARY = re.compile(r"^segments check: (\d+) cases, (\d+) loci, (\d+) runs, (\d+) crossing a word, (\d+) requests, (\d+) refused; (\d+) violations$", re.M)

LOCI = [1, 63, 64, 65, 128, 129, 191, 4096]


def shapes_pedigree():
    """test_link_host's: 1, 2 founders; 3 = (1, 2); 4 = (1, 2); 5 = (3, 4); 6 = (3, 3); 7 = (0, 4); 8 = (5, 7); 9 founder."""
    ind = np.arange(1, 10, dtype=np.int64)
    fa = np.array([0, 0, 1, 1, 3, 3, 0, 5, 0], dtype=np.int64)
    mo = np.array([0, 0, 2, 2, 4, 3, 4, 7, 0], dtype=np.int64)
    return ind, fa, mo


def edge_sets(L):
    """One bin [1, L + 1); every length its own bin (L <= 255); edges that leave lengths in `below` and in `above`; powers of two."""
    sets = [np.array([1, L + 1])]
    if L <= 255:
        sets.append(np.arange(1, L + 2))
    if L >= 4:
        sets.append(np.array([2, 3, max(L // 2, 4)]))
    sets.append(np.array([1, 2, 4, 8, 16, 64, 65, 4097]))
    return [s.astype(np.int32) for s in sets]


def min_locis(L):
    return sorted({1, 2, 64, 65, L, L + 1})


def check_bits(gen, bits, note):
    bits = np.asarray(bits, dtype=np.uint8)
    L = len(bits)
    words = words_of(bits)
    for edges in edge_sets(L):
        for m in min_locis(L):
            want_h, want_p = reduce_bits(bits, edges, m)
            got_h, got_p = gen._capi.seg_host(L, words, edges, m)
            assert np.array_equal(got_h, want_h) and np.array_equal(got_p, want_p), (note, L, edges[:6], m, got_h[got_h[:, 0] > 0], want_h[want_h[:, 0] > 0], got_p, want_p)


@pytest.mark.parametrize("L", LOCI)
def test_host_walk_on_random_words(gen, L):
    rng = np.random.default_rng(100 + L)
    for density in (1 / 64, 1 / 2, 63 / 64):
        for _ in range(6 if L < 4096 else 2):
            check_bits(gen, rng.random(L) < density, "density %g" % density)
    check_bits(gen, np.ones(L), "ones")
    check_bits(gen, np.zeros(L), "zeros")
    check_bits(gen, np.arange(L) % 2, "alternating from 0")
    check_bits(gen, (np.arange(L) + 1) % 2, "alternating from 1")


@pytest.mark.parametrize("L", LOCI)
def test_host_walk_on_the_word_borders(gen, L):
    def run(lo, hi):                         # the loci lo .. hi - 1
        b = np.zeros(L, dtype=np.uint8)
        b[lo:hi] = 1
        return b

    check_bits(gen, run(0, 1), "locus 0 only")
    check_bits(gen, run(L - 1, L), "locus L - 1 only")
    check_bits(gen, run(0, L), "the whole chromosome")
    if L >= 3:
        check_bits(gen, run(1, L - 1), "interior, all but the ends")
    if L >= 65:
        check_bits(gen, run(40, 64), "ends at bit 63, a zero at bit 0 of the next word")
        check_bits(gen, run(0, 64), "the first word exactly")
        check_bits(gen, run(64, min(L, 70)), "starts at bit 0 of the second word")
        check_bits(gen, run(63, 65), "two loci across the border")
        check_bits(gen, run(40, 64) | run(65, min(L, 66)), "a run to bit 63, a gap of one, a run from bit 1")
    if L >= 129:
        check_bits(gen, run(64, 128), "the second word exactly")
        check_bits(gen, run(128, L), "from bit 0 of the third word to the end")
    if L >= 191:
        check_bits(gen, run(60, 130), "a run spanning three words")
        check_bits(gen, run(0, 130), "from locus 0 over three words")
        check_bits(gen, run(60, L), "over three words to the last locus")
    if L == 4096:
        check_bits(gen, run(1, 4095), "4094 loci over 64 words")
        check_bits(gen, run(63, 4033), "from bit 63 of the first word to bit 0 of the last")


def test_odd_W_and_bits_past_L(gen):
    """W = 3: the kernel's last pair of words has an empty second word; genphi_seg_host ignores the bits at and above L."""
    rng = np.random.default_rng(3)
    for L in (129, 150, 191):
        bits = (rng.random(L) < 0.8).astype(np.uint8)
        check_bits(gen, bits, "odd W")
        words = words_of(bits)
        dirty = words.copy()
        dirty[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(L - 128)
        edges = np.array([1, 3, 9, 200], dtype=np.int32)
        a, b = gen._capi.seg_host(L, words, edges, 2), gen._capi.seg_host(L, dirty, edges, 2)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for bad in (dict(loci=0), dict(loci=4097), dict(edges=[3, 3]), dict(edges=[0, 3]), dict(edges=[1, 4098]), dict(edges=[5]), dict(min_loci=0), dict(min_loci=4098),
                dict(any_words=[1, 2])):
        with pytest.raises(ValueError):
            gen._capi.seg_host(**{**dict(loci=64, any_words=[5], edges=[1, 65], min_loci=1), **bad})


@pytest.fixture(scope="module")
def mixed():
    """test_link_host's mixed pedigree: 200 individuals with half-founders and selfing, 12 probands with repeats and a founder; labels
    at S = 40, L = 130."""
    rng = np.random.default_rng(5)
    ind, fa, mo, _ = random_pedigree(rng, 200, p_founder=0.08, p_one_parent=0.1, p_selfing=0.05, max_back=25)
    pro = rng.choice(ind[60:], size=12, replace=False).astype(np.int64)
    pro[9], pro[11], pro[4] = pro[1], pro[1], ind[0]
    return LinkVector(ind, fa, mo, pro).labels(40, 130, 700, 31)


def check_oracle_invariants(labels, edges, groups=None):
    """What the issue asks of the reference on every input it is used with; returns (hist, pairs) at min_loci = 1."""
    n = labels.shape[0]
    s = sums_of(labels)
    hist, pairs = segments_of(labels, edges, 1, groups)
    assert np.array_equal(pairs[..., 0], s[..., 4]) and np.array_equal(pairs[..., 1], s[..., 2])     # the diagonal included
    assert np.array_equal(pairs, pairs.transpose(1, 0, 2)) and np.array_equal(hist, hist.transpose(1, 0, 2, 3))
    if groups is None:
        up = np.triu_indices(n, 1)
        assert hist[0, 0, :, 0].sum() == s[..., 4][up].sum() and hist[0, 0, :, 1].sum() == s[..., 2][up].sum()
    return hist, pairs


def test_invariants_on_the_reference(mixed):
    labels = mixed
    S, L = labels.shape[2], labels.shape[3]
    hist, pairs = check_oracle_invariants(labels, [2, 4, 8, 16, 32, 64])
    assert hist[0, 0, 0, 0] > 0 and hist[0, 0, -1, 0] > 0 and (hist[0, 0, 1:-1, 0] > 0).sum() >= 3
    k = np.arange(12)
    assert np.all(pairs[k, k, 0] == S) and np.all(pairs[k, k, 1] == S * L) and np.all(pairs[k, k, 2] == S * L)
    assert np.all(hist[..., 2] <= hist[..., 0]) and np.all(hist[..., 0] <= hist[..., 1])
    # the longest segment bounds the mean one; min_loci only removes
    h2, p2 = segments_of(labels, [2, 4, 8, 16, 32, 64], 9)
    assert np.array_equal(h2, hist) and np.array_equal(p2[..., 2], pairs[..., 2]) and np.all(p2[..., :2] <= pairs[..., :2]) and np.any(p2[..., 0] < pairs[..., 0])
    assert np.all(p2[..., 1] >= 9 * p2[..., 0])
    # groups: the sum over a <= b is the ungrouped table of the labelled pairs; everyone in one group is no groups
    groups = np.array([0, 1, 2, 0, -1, 1, 1, 0, -1, 1, 0, 1])
    hg, pg = check_oracle_invariants(labels, [2, 4, 8, 16, 32, 64], groups)
    assert hg.shape == (3, 3, 7, 3) and np.array_equal(pg, pairs)
    keep = np.flatnonzero(groups >= 0)
    sub, _ = segments_of(labels[keep], [2, 4, 8, 16, 32, 64])
    assert np.array_equal(sum(hg[a, b] for a in range(3) for b in range(a, 3)), sub[0, 0])
    assert np.all(hg[2, 2] == 0)                                                          # a group with one member has no pair
    one, _ = segments_of(labels, [2, 4, 8, 16, 32, 64], 1, np.zeros(12, dtype=np.int64))
    assert np.array_equal(one, hist)
    c = run_classes(labels)
    assert c["segments"] == hist[0, 0, :, 0].sum() and c["censored"] == hist[0, 0, :, 2].sum() and c["interior"] + c["censored"] == c["segments"]
    assert min(c.values()) > 0, c


def test_argument_errors(gen):
    ind, fa, mo = shapes_pedigree()
    h = gen.SharingPlan(ind, fa, mo, [8, 6, 5, 8], loci=100, q=64, simul_no=10, seed=3)
    ok = dict(edges=[1, 2, 4, 101], min_loci=1, groups=None)

    def ask(match, **kw):
        with pytest.raises(ValueError, match=match):
            h.request_segments(**{**ok, **kw})

    h.request_segments(**ok)
    h.request_segments([1, 4097], 4097, [0, -1, 31, 0])                                   # 528 x 3 cells
    h.request_segments(np.arange(1, 258), 1, None)                                        # 257 edges
    h.request_segments(np.arange(1, 31), 1, [0, 10, -1, 3])                               # 11 groups, 30 edges: 2046 cells, the most that can be asked
    ask("edges\\[2\\] = 2 does not exceed edges\\[1\\] = 2", edges=[1, 2, 2, 5])
    ask("edges\\[1\\] = 3 does not exceed", edges=[5, 3])
    ask("edges\\[0\\] = 0 is below 1", edges=[0, 3])
    ask("edges\\[0\\] = -4", edges=[-4, 3])
    ask("= 4098 is above 4097", edges=[1, 4098])
    ask("258 edges", edges=np.arange(1, 259))
    ask("1 edges", edges=[7])
    ask("0 edges", edges=[])                                                              # edges=None withdraws; an empty list is a mistake
    ask("0 edges", edges=np.zeros(0, dtype=np.int32))
    ask("33 groups", groups=[0, 32, 1, 1])
    ask("2050 cells", edges=np.arange(1, 205), groups=[0, 3, 1, 1])                       # 10 x 205: the fewest cells above 2048 that can be asked
    ask("group\\[1\\] = -2", groups=[0, -2, 1, 1])
    ask("min_loci = 0", min_loci=0)
    ask("min_loci = 4098", min_loci=4098)
    ask("min_loci", min_loci=1 << 40)
    ask("3 labels for 4 probands", groups=[0, 1, 1])
    ask("32-bit integers", edges=[1.5, 3.0])
    ask("32-bit integers", edges=[1, 1 << 40])
    # the C entry points themselves
    L = gen._capi.lib()
    ARG = gen._capi.GENPHI_ERR_ARG
    e = np.array([1, 5], dtype=np.int32)
    ep = e.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert L.genphi_seg_request(None, 2, ep, 1, 0, None) == ARG and L.genphi_seg_to_host(None, None, None) == ARG
    assert L.genphi_seg_stats(None, None, None, None, None, None) == ARG
    assert L.genphi_seg_request(h._h, 2, None, 1, 0, None) == ARG and L.genphi_seg_request(h._h, 2, ep, 1, 2, None) == ARG
    assert L.genphi_seg_request(h._h, -1, ep, 1, 0, None) == ARG and L.genphi_seg_request(h._h, 2, ep, 1, -1, None) == ARG
    assert L.genphi_seg_host(64, None, 2, ep, 1, None, None) == ARG
    # after the errors the handle and its request stand; nothing is computed yet
    with pytest.raises(ValueError, match="nothing computed"):
        h.segments_to_host()
    st = h.segment_stats()
    assert st == dict(segment_ms=0.0, word_ops=0.0, segments=0, cells=0, lds_bytes=0)
    h.request_segments(None)
    h.close()
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(9, dtype=np.int64)}, sort=False)
    for kw in (dict(pro=[]), dict(simulNo=0), dict(loci=0), dict(loci=4097), dict(probRecomb=0.51), dict(bins=[3, 3]), dict(bins=[0, 5]), dict(bins=[]), dict(minLoci=0),
               dict(groups={}), dict(groups={k: k for k in range(1, 10)}, pro=np.arange(1, 10), bins=np.arange(1, 60))):
        with pytest.raises(ValueError):
            gen.simuSegments(ped, **kw)
    with pytest.raises(KeyError):
        gen.simuSegments(ped, pro=[77])


def test_symbols_are_exported_declared_and_bound(gen):
    from genlib_jl_amd import _capi
    header = open(os.path.join(ROOT, "include", "genphi.h")).read()
    L = ctypes.CDLL(_capi.LIB_PATH)
    names = ["genphi_seg_" + n for n in ("request", "to_host", "stats", "host")]
    for name in names:
        assert hasattr(L, name) and name in _capi.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, header), name
    assert sum(n.startswith("genphi_seg_") for n in _capi.EXPORTED_SYMBOLS) == 4
    lib = _capi.lib()
    assert [len(getattr(lib, n).argtypes) for n in names] == [6, 3, 6, 7]
    for macro, value in (("GENPHI_SEG_MAX_EDGES", 257), ("GENPHI_SEG_MAX_EDGE", 4097), ("GENPHI_SEG_MAX_GROUPS", 32), ("GENPHI_SEG_MAX_CELLS", 2048)):
        assert re.search(r"#define %s %d\b" % (macro, value), header) and getattr(_capi, macro) == value
    assert gen.simuSegments.__doc__ and gen.SimuSegments.__doc__ and gen.SharingPlan.request_segments.__doc__


def test_SimuSegments_properties(gen):
    """Every property from hand-made integers."""
    S, L = 10, 8
    sums = np.zeros((2, 2, 6), dtype=np.int64)
    sharing = gen.SimuSharing(np.array([5, 6]), sums, L, 64, S, 1, None, None)
    edges = np.array([2, 4, 8], dtype=np.int32)
    hist = np.zeros((1, 1, 4, 3), dtype=np.int64)
    hist[0, 0] = [[7, 7, 2], [4, 10, 1], [0, 0, 0], [3, 24, 3]]                            # below, [2, 4), [4, 8), above
    pairs = np.zeros((2, 2, 3), dtype=np.int64)
    pairs[0, 1] = pairs[1, 0] = [7, 34, 50]
    pairs[0, 0] = pairs[1, 1] = [S, S * L, S * L]
    r = gen.SimuSegments(np.array([5, 6]), edges, 2, hist, pairs, sharing)
    assert r.counts.tolist() == [4, 0] and r.loci_in.tolist() == [10, 0] and r.censored.tolist() == [1, 0]
    assert r.below.tolist() == [7, 7, 2] and r.above.tolist() == [3, 24, 3] and r.names is None and r.sizes is None
    assert r.mean_length[0] == 2.5 and np.isnan(r.mean_length[1])
    assert r.segments_over[0, 1] == 0.7 and r.loci_over[0, 1] == 3.4 and r.longest[0, 1] == 5.0 and r.longest[1, 1] == 8.0
    assert r.locus_cM == -50.0 * np.log(1.0 - 128 / 65536.0) and r.minLoci == 2 and r.sharing is sharing and "14 segments" in repr(r)
    assert gen.SimuSegments(np.array([5]), edges, 1, hist, pairs, gen.SimuSharing(np.array([5]), sums, L, 32768, S, 1, None, None)).locus_cM == np.inf
    assert gen.SimuSegments(np.array([5]), edges, 1, hist, pairs, gen.SimuSharing(np.array([5]), sums, L, 0, S, 1, None, None)).locus_cM == 0.0
    hg = np.zeros((2, 2, 4, 3), dtype=np.int64)
    hg[0, 1] = hg[1, 0] = hist[0, 0]
    hg[1, 1, 2] = [5, 25, 0]
    g = gen.SimuSegments(np.array([5, 6, 7]), edges, 1, hg, np.zeros((3, 3, 3), dtype=np.int64), sharing, ["a", "b"], np.array([1, 2]))
    assert g.counts.shape == (2, 2, 2) and g.counts[0, 1].tolist() == [4, 0] and g.counts[1, 1].tolist() == [0, 5] and g.below.shape == (2, 2, 3)
    assert g.mean_length[1, 1, 1] == 5.0 and np.isnan(g.mean_length[0, 0, 0]) and g.above[1, 0].tolist() == [3, 24, 3] and "19 segments, 2 groups" in repr(g)
    # the default edges: 1, 2, 4, .. up to and including the first power of two above loci
    from genlib_jl_amd import _segment_edges
    assert _segment_edges(None, 1024).tolist() == [1 << k for k in range(12)] and _segment_edges(None, 1023).tolist() == [1 << k for k in range(11)]
    assert _segment_edges(None, 1).tolist() == [1, 2] and _segment_edges(None, 5).tolist() == [1, 2, 4, 8] and _segment_edges(None, 4095).tolist() == [1 << k for k in range(13)]
    # 4096: the first power of two above is 8192, past the largest edge; the list ends 4096, 4097 and the last bin is the whole chromosome
    assert _segment_edges(None, 4096).tolist() == [1 << k for k in range(13)] + [4097]


@pytest.mark.parametrize("L", [1, 2, 1023, 1024, 4095, 4096])
def test_the_default_edges_are_a_request_the_library_takes(gen, L):
    """No length lies outside the default bins: the first edge is 1 and the last exceeds L; genphi_seg_request and genphi_seg_host take
    them, loci = 4096 included."""
    from genlib_jl_amd import _segment_edges
    ind, fa, mo = shapes_pedigree()
    edges = _segment_edges(None, L)
    assert edges.dtype == np.int32 and edges[0] == 1 and edges[-1] > L and edges[-2] <= L and np.all(np.diff(edges) > 0) and edges[-1] <= 4097
    h = gen.SharingPlan(ind, fa, mo, [8, 6, 5], loci=L, q=64, simul_no=3, seed=1)
    try:
        h.request_segments(edges)
        h.request_segments(edges, L + 1, [0, 1, -1])
    finally:
        h.close()
    bits = np.ones(L, dtype=np.uint8)
    hist, pair = gen._capi.seg_host(L, words_of(bits), edges, 1)
    assert hist[-2].tolist() == [1, L, 1] and hist[:-2].sum() == 0 and hist[-1].sum() == 0 and pair.tolist() == [1, L, L]     # the last bin, not `above`


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_host_code_as_a_stand_alone_program(san, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "segments_check")
    flags = ["-O2"] if san is None else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra"] + flags + [os.path.join(ROOT, "tests", "segments_check.cpp"), "-o", exe]
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
    cases, loci, runs, crossing, requests, refused, violations = (int(v) for v in m.groups())
    assert violations == 0 and cases == 100_000 and loci > 10_000_000 and runs > 1_000_000 and crossing > 50_000 and requests == 600 and 100 < refused < 500
    assert "VIOLATION" not in run.stderr and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-3000:]
