"""gen.simuSegments on the MI355X (gen.SharingPlan.request_segments, gen.simuSegments) against the reference of
tests/segments_oracle.py on the labels of tests/link_oracle.py: every comparison is np.array_equal, and every handle is computed
twice with equal bytes.  Shapes are the smallest at which link_segment_kernel (csrc/link.hip) and the walk it carries from word to
word (csrc/link_segments.h) can go wrong: chromosomes at the word and pair edges, every lanes-per-simulation form, runs over all 64
words, forced and ragged panels, probands at the tile edges, groups with -1, with one member and with everyone, repeats and
half-founders, and the largest table that can be asked for.  On every input the reference itself is first held against the sums of
link_oracle.sums_of (tests/test_segments_host.py: check_oracle_invariants)."""
import numpy as np
import pytest

from link_oracle import LinkVector, sums_of
from segments_oracle import run_classes, segments_of
from test_link_gpu import generated_clan
from test_segments_host import check_oracle_invariants

pytestmark = pytest.mark.gpu

EDGES_129 = [2, 4, 8, 16, 32, 64, 100]       # the main case: lengths of 1 in `below`, of 100 .. 129 in `above`


def _args(ped):
    return ped.ind, ped.father, ped.mother


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b), (np.argwhere(a != b)[:5], a[a != b][:5], b[a != b][:5])


def _check(gen, args, pro, L, q, S, seed, edges, min_loci=1, groups=None, want=None, **kw):
    """The table and the pair sums of one handle, computed twice, against the reference on the labels want (n_pro, 2, >= S, L);
    returns (hist, pairs, segment_stats())."""
    if want is None:
        want = LinkVector(*args, pro).labels(S, L, q, seed)
    want = np.ascontiguousarray(want[:, :, :S])
    check_oracle_invariants(want, edges, groups)
    hist, pairs = segments_of(want, edges, min_loci, groups)
    sums = sums_of(want)
    h = gen.SharingPlan(*args, pro, loci=L, q=q, simul_no=S, seed=seed, **kw)
    try:
        h.request_segments(edges, min_loci, groups)
        for _ in range(2):
            h.compute()
            got_hist, got_pairs = h.segments_to_host()
            _same(got_hist, hist)
            _same(got_pairs, pairs)
            _same(h.sums_to_host(), sums)
        st = h.segment_stats()
        G = hist.shape[0]
        cells = G * (G + 1) // 2 * (len(edges) + 1)
        n, W = len(pro), (L + 63) // 64
        upper = np.triu(np.ones((G, G), dtype=bool))
        assert st["segment_ms"] > 0.0 and st["cells"] == cells and st["lds_bytes"] == 2048 * h.planes + 24 * cells + 4 * len(edges)
        assert st["segments"] == hist[upper][..., 0].sum() and st["word_ops"] == n * (n + 1) // 2 * S * W * (8 * h.planes + 10)
        return hist, pairs, st
    finally:
        h.close()


@pytest.fixture(scope="module")
def ji(gen):
    ped = gen.genealogy(gen.geneaJi)
    return ped, gen.pro(ped)


@pytest.fixture(scope="module")
def clan():
    """test_link_gpu's clan: 132 individuals in few generations, with its random order to draw probands from."""
    args = generated_clan(12, 24, 5, 11)
    return args, np.random.default_rng(4).permutation(args[0])


@pytest.fixture(scope="module")
def main_case(clan):
    """The first 40 probands of the clan at S = 7, L = 129, q = 700, seed 9: the reference labels, computed once."""
    args, order = clan
    pro = order[:40]
    return args, pro, LinkVector(*args, pro).labels(7, 129, 700, 9)


def test_the_main_case_reaches_every_class_of_run(main_case):
    """On the reference alone: a change of fixture must not quietly empty the tests below."""
    _, _, want = main_case
    c = run_classes(want)
    print("main case:", c)
    assert min(c.values()) > 0 and c["lengths"] >= 20, c
    hist, _ = segments_of(want, EDGES_129)
    assert hist[0, 0, 0, 0] > 0 and hist[0, 0, -1, 0] > 0 and (hist[0, 0, 1:-1, 0] > 0).sum() >= 3
    assert hist[0, 0, :, 0].sum() == c["segments"] and hist[0, 0, :, 2].sum() == c["censored"]


@pytest.mark.parametrize("all_pairs", [False, True])
def test_main_case_with_forced_panels(gen, main_case, all_pairs):
    """Panels of 1, 3 and 7 simulations and the default at S = 7 (3: a ragged last panel); 40 probands are two tiles."""
    args, pro, want = main_case
    seen = []
    for sims, panels in ((1, 7), (3, 3), (7, 1), (0, 1)):
        hist, pairs, _ = _check(gen, args, pro, 129, 700, 7, 9, EDGES_129, 5, want=want, panel_sims=sims, all_pairs=all_pairs)
        seen.append((hist, pairs))
    assert all(np.array_equal(h, seen[0][0]) and np.array_equal(p, seen[0][1]) for h, p in seen)


@pytest.mark.parametrize("L", [1, 63, 64, 65, 128, 129, 191])
def test_word_edges(gen, ji, L):
    """An odd W (L = 1, 63, 64, 129, 191) leaves the second word of the last pair empty."""
    ped, pro = ji
    o = LinkVector(*_args(ped), pro)
    edges = sorted({1, 2, 3, max(L // 2, 4), max(L, 5), L + 5})
    for q in (0, 1, 0x5555, 32768):
        want = o.labels(64, L, q, 2024)
        for S in (1, 3, 64):
            _check(gen, _args(ped), pro, L, q, S, 2024, edges, min(2, L), want=want)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 65])
def test_probands_at_the_tile_edges(gen, clan, n):
    args, order = clan
    pro = order[:n]
    groups = (np.arange(n) % 3 - (np.arange(n) % 5 == 0)).clip(-1)                        # -1, 0, 1, 2 across the tiles
    want = LinkVector(*args, pro).labels(2, 65, 2000, 5)
    for all_pairs in (False, True):
        _check(gen, args, pro, 65, 2000, 2, 5, [1, 2, 3, 5, 9, 17, 33, 66], 3, want=want, all_pairs=all_pairs)
    _check(gen, args, pro, 65, 2000, 2, 5, [2, 5, 9, 33], 1, groups, want=want)


@pytest.mark.parametrize("words", [1, 2, 3, 4, 8, 16, 32, 64])
def test_every_lanes_per_simulation_form(gen, ji, words):
    """q = 64: runs longer than a word, carried from word to word; q = 1024: several runs in a word."""
    ped, pro = ji
    L = 64 * words
    for q in (64, 1024):
        _check(gen, _args(ped), pro, L, q, 3, 31, [1, 2, 8, 64, 65, 129, 1000, 4097], 64)


@pytest.mark.parametrize("q", [1, 64])
def test_long_segments_across_word_borders(gen, q):
    """test_link_gpu's sibs at L = 4096: a child shares one allele with its parent at every locus, one segment of 64 words that a walk
    which lost the carry would cut into 64; two sibs share in few, long segments."""
    ind = np.arange(1, 6, dtype=np.int64)
    fa = np.array([0, 0, 1, 1, 0], dtype=np.int64)
    mo = np.array([0, 0, 2, 2, 0], dtype=np.int64)
    S, L = 4, 4096
    want = LinkVector(ind, fa, mo, ind).labels(S, L, q, 12)
    c = run_classes(want)
    print("sibs at q = %d:" % q, c)
    assert c["cross"] > 0 and c["spanning"] > 0
    if q == 64:
        assert c["interior"] > 0 and c["segments"] > c["spanning"] and c["cross"] >= c["segments"] // 2
    hist, pairs, _ = _check(gen, (ind, fa, mo), ind, L, q, S, 12, [1, 64, 65, 128, 1024, 4096, 4097], 65, want=want)
    assert pairs[0, 2].tolist() == [S, S * L, S * L] and pairs[0, 4].tolist() == [0, 0, 0]
    assert hist[0, 0, -2, 0] == c["spanning"] and hist[0, 0, -1, 0] == 0                  # [4096, 4097): the whole chromosome


def test_groups(gen, main_case):
    args, pro, want = main_case
    n = len(pro)
    groups = np.arange(n) % 3
    groups[[0, 7, 21, 39]] = -1
    groups[groups == 2] = 1
    groups[5] = 2                                                                         # a group with one member
    hist, pairs, _ = _check(gen, args, pro, 129, 700, 7, 9, EDGES_129, 1, groups, want=want)
    assert hist.shape == (3, 3, 8, 3) and np.array_equal(hist, hist.transpose(1, 0, 2, 3)) and np.all(hist[2, 2] == 0) and hist[0, 2].any()
    keep = np.flatnonzero(groups >= 0)
    plain, plain_pairs, _ = _check(gen, args, pro[keep], 129, 700, 7, 9, EDGES_129, 1, want=np.ascontiguousarray(want[keep]))
    _same(sum(hist[a, b] for a in range(3) for b in range(a, 3)), plain[0, 0])            # the labelled pairs, ungrouped
    _same(np.ascontiguousarray(pairs[np.ix_(keep, keep)]), plain_pairs)                   # the pair sums take no notice of the labels
    one, _, _ = _check(gen, args, pro, 129, 700, 7, 9, EDGES_129, 1, np.zeros(n, dtype=np.int64), want=want)
    none, _, _ = _check(gen, args, pro, 129, 700, 7, 9, EDGES_129, 1, want=want)
    _same(one, none)                                                                      # everyone in one group is no groups
    nobody, _, _ = _check(gen, args, pro, 129, 700, 7, 9, EDGES_129, 1, np.full(n, -1), want=want)
    assert nobody.shape == (1, 1, 8, 3) and not nobody.any()


def test_cross_checks_with_no_oracle(gen, clan):
    """One bin [1, L + 1) and min_loci = 1: the device's pairs[..., :2] are its own sums[..., [4, 2]] and the table is their sum over
    i < j; the censored segments are at most two per pair and simulation."""
    args, order = clan
    pro, L, S = order[:70], 200, 9
    h = gen.SharingPlan(*args, pro, loci=L, q=900, simul_no=S, seed=77, panel_sims=4)
    try:
        h.request_segments([1, L + 1])
        for _ in range(2):
            h.compute()
            hist, pairs = h.segments_to_host()
            sums = h.sums_to_host()
            _same(np.ascontiguousarray(pairs[..., :2]), np.ascontiguousarray(sums[..., [4, 2]]))
            up = np.triu_indices(len(pro), 1)
            assert hist.shape == (1, 1, 3, 3) and not hist[0, 0, 0].any() and not hist[0, 0, 2].any()
            assert hist[0, 0, 1, 0] == sums[..., 4][up].sum() and hist[0, 0, 1, 1] == sums[..., 2][up].sum()
            assert 0 < hist[0, 0, 1, 2] <= 2 * S * len(up[0]) and np.all(pairs[..., 2] * np.maximum(pairs[..., 0], 1) >= pairs[..., 1])
            assert np.array_equal(pairs, pairs.transpose(1, 0, 2)) and np.all(pairs[..., 2] <= pairs[..., 1])
        assert h.stats()["panels"] == 3 and h.segment_stats()["segments"] == hist[0, 0, 1, 0]
    finally:
        h.close()


def test_repeats_and_half_founders(gen):
    """1, 2 founders; 3 = (1, 2); 4 = (1, 2); 5 = (3, 4) inbred; 6 = (3, 3) selfed; 7 = (0, 4) half-founder; 8 = (5, 7); 9 founder."""
    ind = np.arange(1, 10, dtype=np.int64)
    fa = np.array([0, 0, 1, 1, 3, 3, 0, 5, 0], dtype=np.int64)
    mo = np.array([0, 0, 2, 2, 4, 3, 4, 7, 0], dtype=np.int64)
    pro = np.array([8, 6, 8, 7, 5, 1, 9, 6], dtype=np.int64)
    S, L = 40, 200
    hist, pairs, _ = _check(gen, (ind, fa, mo), pro, L, 500, S, 4, [1, 3, 10, 30, 100, 200, 201], 10, [0, 1, 0, 1, -1, 0, 1, 1])
    assert np.array_equal(pairs[0, 2], pairs[0, 0]) and pairs[0, 0].tolist() == [S, S * L, S * L]       # repeats of one ID: the whole chromosome
    assert not pairs[6][[0, 1, 2, 3, 4, 5, 7]].any()                                                  # 9 is unrelated
    assert hist[0, 0, -2, 0] >= S                                                                     # the pair of the two 8s: S segments of L loci


def test_no_side_effects_second_request_and_withdrawal(gen, main_case):
    args, pro, want = main_case
    want = np.ascontiguousarray(want[:, :, :4])
    h = gen.SharingPlan(*args, pro, loci=129, q=700, simul_no=4, seed=9, labels=True)
    try:
        h.compute()
        with pytest.raises(ValueError, match="without a request"):
            h.segments_to_host()
        sums, labels = h.sums_to_host(), h.labels_to_host()
        _same(labels, want)
        assert h.segment_stats() == dict(segment_ms=0.0, word_ops=0.0, segments=0, cells=0, lds_bytes=0)
        h.request_segments(EDGES_129, 3)
        h.compute()
        assert sums.tobytes() == h.sums_to_host().tobytes() and labels.tobytes() == h.labels_to_host().tobytes()
        first = h.segments_to_host()
        _same(first[0], segments_of(want, EDGES_129, 3)[0])
        _same(first[1], segments_of(want, EDGES_129, 3)[1])
        with pytest.raises(ValueError, match="does not exceed"):
            h.request_segments([4, 4])                                                    # a refused request changes nothing
        groups = np.arange(len(pro)) % 4
        h.request_segments([1, 10, 130], 20, groups)                                      # takes effect at the next compute only
        _same(h.segments_to_host()[0], first[0])
        h.compute()
        second = h.segments_to_host()
        _same(second[0], segments_of(want, [1, 10, 130], 20, groups)[0])
        _same(second[1], segments_of(want, [1, 10, 130], 20, groups)[1])
        assert sums.tobytes() == h.sums_to_host().tobytes() and labels.tobytes() == h.labels_to_host().tobytes()
        h.request_segments(None)
        _same(h.segments_to_host()[0], second[0])                                         # until the next compute
        h.compute()
        with pytest.raises(ValueError, match="without a request"):
            h.segments_to_host()
        assert gen._capi.lib().genphi_seg_to_host(h._h, None, None) == gen._capi.GENPHI_ERR_ARG
        assert sums.tobytes() == h.sums_to_host().tobytes() and h.segment_stats()["cells"] == 0
    finally:
        h.close()


def test_simuSegments_on_geneaJi_with_groups(gen):
    ped = gen.genealogy(gen.geneaJi)
    pro = np.concatenate([gen.pro(ped), [25, 18, 27, 26]]).astype(np.int64)
    groups = {int(i): ("north" if k % 2 else "south") for k, i in enumerate(pro[:-1])}   # 26 is in no group; "west" has no proband
    groups[999] = "west"
    kw = dict(loci=150, probRecomb=0.02, simulNo=30, seed=7)
    r = gen.simuSegments(ped, pro, minLoci=4, groups=groups, **kw)
    labels = np.array([1, 0, 1, 0, 1, 0, -1])                                             # names sorted: north, south, west
    want = LinkVector(*_args(ped), pro).labels(30, 150, r.sharing.q, 7)
    hist, pairs = segments_of(want, r.edges, 4, labels)
    assert r.names == ["north", "south", "west"] and r.sizes.tolist() == [3, 3, 0] and r.edges.tolist() == [1, 2, 4, 8, 16, 32, 64, 128, 256]
    assert r.counts.shape == (3, 3, 8) and not r.counts[2].any() and not r.counts[:, 2].any() and r.minLoci == 4
    _same(np.ascontiguousarray(r.counts[:2, :2]), np.ascontiguousarray(hist[..., 1:-1, 0]))
    _same(np.ascontiguousarray(r.loci_in[:2, :2]), np.ascontiguousarray(hist[..., 1:-1, 1]))
    _same(np.ascontiguousarray(r.censored[:2, :2]), np.ascontiguousarray(hist[..., 1:-1, 2]))
    _same(np.ascontiguousarray(r.below[:2, :2]), np.ascontiguousarray(hist[..., 0, :]))
    _same(np.ascontiguousarray(r.above[:2, :2]), np.ascontiguousarray(hist[..., -1, :]))
    _same(r.pairs, pairs)
    _same(r.pro, pro)
    sharing = gen.simuSharing(ped, pro, **kw)
    _same(r.sharing.sums, sharing.sums)
    _same(r.sharing.sums, sums_of(want))
    assert (r.sharing.q, r.sharing.seed, r.sharing.simulNo, r.sharing.loci) == (sharing.q, 7, 30, 150) and r.locus_cM == -50.0 * np.log(1 - 2 * sharing.q / 65536)
    assert r.longest[3, 4] == 150.0 and r.segments_over[3, 4] == 1.0 and r.loci_over[3, 4] == 150.0      # 25 is the father of 18
    plain = gen.simuSegments(ped, pro, bins=[1, 10, 151], **kw)
    assert plain.names is None and plain.counts.shape == (2,) and plain.below.tolist() == [0, 0, 0] and plain.above.tolist() == [0, 0, 0]
    _same(plain.counts, segments_of(want, [1, 10, 151])[0][0, 0, 1:-1, 0])
    assert plain.mean_length[1] >= 10.0


def test_simuSegments_with_default_bins_at_the_widest_chromosome(gen, ji):
    """loci = 4096, everything else at its default: the edges end 2048, 4096, 4097, the whole chromosome is the last bin and `above`
    is empty."""
    ped, pro = ji
    r = gen.simuSegments(ped, loci=4096, simulNo=2, seed=5)
    assert r.edges.tolist() == [1 << k for k in range(13)] + [4097] and r.counts.shape == (13,)
    want = LinkVector(*_args(ped), pro).labels(2, 4096, r.sharing.q, 5)
    hist, pairs = segments_of(want, r.edges)
    _same(r.counts, np.ascontiguousarray(hist[0, 0, 1:-1, 0]))
    _same(r.loci_in, np.ascontiguousarray(hist[0, 0, 1:-1, 1]))
    _same(r.censored, np.ascontiguousarray(hist[0, 0, 1:-1, 2]))
    _same(r.pairs, pairs)
    _same(r.sharing.sums, sums_of(want))
    assert r.below.tolist() == [0, 0, 0] and r.above.tolist() == [0, 0, 0] and r.counts.sum() > 0 and np.all(r.longest[[0, 1, 2], [0, 1, 2]] == 4096.0)


def test_the_largest_table(gen, main_case):
    """G (G + 1) / 2 x (n_bins + 2) is never 2,048 or 2,049 for 2 .. 257 edges: the most cells a request can have is 2,046 (11 groups, 30
    edges) and the fewest it is refused with 2,050 (4 groups, 204 edges)."""
    args, pro, want = main_case
    edges = list(range(1, 25)) + [30, 40, 60, 90, 120, 129]
    groups = np.arange(len(pro)) % 11
    hist, _, st = _check(gen, args, pro, 129, 700, 7, 9, edges, 1, groups, want=want)
    assert st["cells"] == 2046 and hist.shape == (11, 11, 31, 3) and (hist[..., 0] > 0).sum() > 500
    h = gen.SharingPlan(*args, pro, loci=129, q=700, simul_no=7, seed=9)
    try:
        with pytest.raises(ValueError, match="2050 cells"):
            h.request_segments(np.arange(1, 205), 1, np.arange(len(pro)) % 4)
    finally:
        h.close()
