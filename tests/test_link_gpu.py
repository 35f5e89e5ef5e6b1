"""gen.simuSharing on the MI355X (gen.SharingPlan, gen.simuSharing) against the reference of tests/link_oracle.py: every comparison
is np.array_equal.  The labels are compared with the reference's, and the sums with sums_of of the device's own labels and with
sums_of of the reference's; every handle is computed twice with equal bytes.  Shapes are the smallest at which each part of
csrc/link.hip can go wrong: chromosomes at the word and pair edges, the widest chromosome, every lanes-per-simulation form of the step
kernel, forced and ragged panels, probands at the pair kernel's tile edges, long child lists, deep chains, half-founders, selfing and
repeats, and segments that run across word borders.  A reference is computed once per (pedigree, L, q) at the largest S and cut to
the simulations a case needs (the prefix rule of the definition, checked on the reference itself in tests/test_link_host.py)."""
import numpy as np
import pytest

from exact_kinship import ExactKinship
from link_oracle import LinkVector, sums_of

pytestmark = pytest.mark.gpu


def _args(ped):
    return ped.ind, ped.father, ped.mother


def _ped(gen, ind, fa, mo):
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b), np.argwhere(a != b)[:5]


def _blocks_per_side(L, q):
    W = (L + 63) // 64
    first = 8 if q == 0 else ((q & -q).bit_length() - 1) // 2
    return W * (8 - first) + 1


def _check(gen, args, pro, L, q, S, seed, want=None, labels=True, **kw):
    """Sums and labels of one handle, computed twice, against the reference labels want (n_pro, 2, >= S, L); returns stats()."""
    o = LinkVector(*args, pro)
    if want is None:
        want = o.labels(S, L, q, seed)
    want = np.ascontiguousarray(want[:, :, :S])
    sums = sums_of(want)
    h = gen.SharingPlan(*args, pro, loci=L, q=q, simul_no=S, seed=seed, labels=labels, **kw)
    try:
        for _ in range(2):
            h.compute()
            got = h.sums_to_host()
            if labels:
                mine = h.labels_to_host()
                _same(mine, want)
                _same(got, sums_of(mine))
            else:
                with pytest.raises(ValueError):
                    h.labels_to_host()
            _same(got, sums)
        st = h.stats()
        assert st["sweep_ms"] >= 0.0 and st["pair_ms"] > 0.0
        n, W = len(pro), (L + 63) // 64
        pairs = n * n if kw.get("all_pairs") else n * (n + 1) // 2
        known = 2 * o.n_live - o.n_labels
        assert st["word_ops"] == pairs * S * W * (8 * h.planes + 32) and st["planes"] == h.planes == o.planes and st["levels"] == o.levels
        assert st["philox_blocks"] == known * S * _blocks_per_side(L, q) and st["algorithmic_bytes"] == 48 * o.planes * known * S * ((W + 1) // 2)
        assert (st["tile_rows"], st["tile_cols"]) == (32, 32)
        return st
    finally:
        h.close()


@pytest.fixture(scope="module")
def ji(gen):
    ped = gen.genealogy(gen.geneaJi)
    return ped, gen.pro(ped)


def generated_clan(n_founders, per_generation, generations, seed):
    """A clan of this file's own: founders, then generations whose members take a father and a mother among the two generations
    before them (now and then the same individual twice, now and then one parent only).  IDs ascend with the generations."""
    rng = np.random.default_rng(seed)
    ind, fa, mo = list(range(1, n_founders + 1)), [0] * n_founders, [0] * n_founders
    older, last = [], list(ind)
    for _ in range(generations):
        pool, new = older + last, []
        for _ in range(per_generation):
            f, m = (int(x) for x in rng.choice(pool, size=2))
            u = rng.random()
            if u < 0.05:
                m = f
            elif u < 0.10:
                m = 0
            elif u < 0.15:
                f = 0
            new.append(len(ind) + 1)
            ind.append(new[-1])
            fa.append(f)
            mo.append(m)
        older, last = last, new
    return np.array(ind, dtype=np.int64), np.array(fa, dtype=np.int64), np.array(mo, dtype=np.int64)


@pytest.fixture(scope="module")
def clan():
    """132 individuals in few generations, closely related, with a random order of them to draw probands from."""
    args = generated_clan(12, 24, 5, 11)
    return args, np.random.default_rng(4).permutation(args[0])


@pytest.mark.parametrize("L", [1, 63, 64, 65, 128, 129, 191])
def test_word_edges(gen, ji, L):
    """An odd W (L = 1, 63, 64, 129, 191) leaves the second word of the last pair empty."""
    ped, pro = ji
    o = LinkVector(*_args(ped), pro)
    for q in (0, 1, 0x5555, 32768):
        want = o.labels(64, L, q, 2024)
        for S in (1, 2, 3, 64):
            st = _check(gen, _args(ped), pro, L, q, S, 2024, want=want)
            assert (st["panels"], st["panel_sims"], st["lanes_per_sim"]) == (1, S, 1 if L <= 128 else 2)
        if q == 0x5555 and L > 1:
            assert len(np.unique(want[0, 0, 0])) > 1                                   # the chromosome is a mosaic


def test_widest_chromosome(gen, ji):
    ped, pro = ji
    st = _check(gen, _args(ped), pro, 4096, 64, 2, 5)
    assert st["lanes_per_sim"] == 32


@pytest.mark.parametrize("words", [1, 2, 3, 4, 8, 16, 32, 64])
def test_every_lanes_per_simulation_form(gen, ji, words):
    ped, pro = ji
    lanes = 1
    while lanes < (words + 1) // 2:
        lanes *= 2
    for q in (1024, 0x5555):
        st = _check(gen, _args(ped), pro, 64 * words, q, 3, 31)
        assert st["lanes_per_sim"] == lanes and st["panel_sims"] == 3


@pytest.mark.parametrize("all_pairs", [False, True])
def test_forced_panels(gen, clan, all_pairs):
    """Panels of 1 and of 3 simulations at S = 7 (a ragged last panel), and the default; 40 probands are two tiles."""
    args, order = clan
    pro = order[:40]
    want = LinkVector(*args, pro).labels(7, 129, 700, 9)
    for sims, panel_sims, panels in ((1, 1, 7), (3, 3, 3), (7, 7, 1), (1000, 7, 1), (0, 7, 1)):
        st = _check(gen, args, pro, 129, 700, 7, 9, want=want, labels=sims != 1, panel_sims=sims, all_pairs=all_pairs)
        assert (st["panel_sims"], st["panels"]) == (panel_sims, panels)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 65, 99])
def test_probands_at_the_tile_edges(gen, clan, n):
    args, order = clan
    pro = order[:n]
    want = LinkVector(*args, pro).labels(2, 65, 2000, 5)
    for all_pairs in (False, True):
        _check(gen, args, pro, 65, 2000, 2, 5, want=want, all_pairs=all_pairs, labels=not all_pairs)
    s = sums_of(want)
    assert np.array_equal(s, s.transpose(1, 0, 2))


def test_hub_couple_with_300_children(gen):
    ind = np.arange(1, 303, dtype=np.int64)
    fa = np.where(ind > 2, 1, 0).astype(np.int64)
    mo = np.where(ind > 2, 2, 0).astype(np.int64)
    st = _check(gen, (ind, fa, mo), ind, 65, 3000, 2, 3)
    assert st["levels"] == 2 and st["planes"] == 2


def test_chain_of_300_levels(gen):
    n = 300
    ind = np.arange(1, 2 * n, dtype=np.int64)            # 1; then (mate, child) pairs: child k = (previous child, mate)
    fa, mo = np.zeros(2 * n - 1, dtype=np.int64), np.zeros(2 * n - 1, dtype=np.int64)
    prev = 1
    for k in range(1, n):
        mate, child = 2 * k, 2 * k + 1
        fa[child - 1], mo[child - 1] = (prev, mate) if k % 2 else (mate, prev)
        prev = child
    pro = np.array([3, 5, 21, 2 * n - 1, 2, 1], dtype=np.int64)
    st = _check(gen, (ind, fa, mo), pro, 130, 3000, 3, 8)
    assert st["levels"] == n and st["planes"] == 10


def test_half_founders_selfing_and_repeated_probands(gen):
    """1, 2 founders; 3 = (1, 2); 4 = (1, 2); 5 = (3, 4) inbred; 6 = (3, 3) selfed; 7 = (0, 4) half-founder; 8 = (5, 7); 9 founder."""
    ind = np.arange(1, 10, dtype=np.int64)
    fa = np.array([0, 0, 1, 1, 3, 3, 0, 5, 0], dtype=np.int64)
    mo = np.array([0, 0, 2, 2, 4, 3, 4, 7, 0], dtype=np.int64)
    pro = np.array([8, 6, 8, 7, 5, 1, 9, 6], dtype=np.int64)
    S, L = 40, 200
    want = LinkVector(ind, fa, mo, pro).labels(S, L, 500, 4)
    _check(gen, (ind, fa, mo), pro, L, 500, S, 4, want=want)
    s = sums_of(want)
    assert np.array_equal(s[0, 2], s[0, 0]) and np.array_equal(s[2, 1], s[0, 1])              # repeats of one ID
    assert not np.array_equal(want[1, 0], want[1, 1])                                         # 6 = (3, 3): the two sides drew their own words
    assert np.all(s[6][[0, 1, 2, 3, 4, 5, 7]] == 0) and s[6, 6].tolist() == [2 * S * L, 4 * S * L * L, S * L, S * L, S, S]   # 9 is unrelated


def test_sub_list_branching_other_seeds_and_prefix(gen, clan):
    (ind, fa, mo), order = clan
    pro = order[:40]
    ped = _ped(gen, ind, fa, mo)
    kw = dict(loci=100, probRecomb=0.01, simulNo=100, seed=9)
    full = gen.simuSharing(ped, pro, labels=True, **kw)
    assert full.sums.dtype == np.int64 and full.sums.shape == (40, 40, 6) and (full.simulNo, full.seed, full.loci, full.q) == (100, 9, 100, 655)
    assert full.probRecomb == 655 / 65536
    want = LinkVector(ind, fa, mo, pro).labels(100, 100, 655, 9)
    _same(full.labels, want)
    _same(full.sums, sums_of(want))
    _same(full.alleles, LinkVector(ind, fa, mo, pro).alleles)
    assert np.array_equal(full.sums, full.sums.transpose(1, 0, 2))
    sub = np.array([33, 3, 3, 17, 7, 39])
    part = gen.simuSharing(ped, pro[sub], **kw)
    _same(part.sums, np.ascontiguousarray(full.sums[np.ix_(sub, sub)]))
    assert part.labels is None and len(part.alleles) < len(full.alleles)
    pruned = gen.branching(ped, pro=pro)
    assert len(pruned) < len(ped)
    again = gen.simuSharing(pruned, pro, labels=True, **kw)
    _same(again.sums, full.sums)
    _same(again.labels, full.labels)
    short = gen.simuSharing(ped, pro, labels=True, **{**kw, "simulNo": 3})
    _same(short.labels, np.ascontiguousarray(full.labels[:, :, :3]))
    assert not np.array_equal(gen.simuSharing(ped, pro, **{**kw, "seed": 10}).sums, full.sums)
    a, b = gen.simuSharing(ped, pro, loci=64, simulNo=8), gen.simuSharing(ped, pro, loci=64, simulNo=8)
    assert a.seed != b.seed and not np.array_equal(a.sums, b.sums)                        # fresh seeds
    dflt = gen.simuSharing(ped, loci=70, length=2.0, simulNo=5, seed=1)                   # pro(ped); Haldane's map
    _same(dflt.pro, gen.pro(ped))
    assert dflt.q == round(65536 * 0.5 * (1 - np.exp(-4.0 / 69)))
    _same(dflt.sums, sums_of(LinkVector(ind, fa, mo, gen.pro(ped)).labels(5, 70, dflt.q, 1)))


def test_no_recombination(gen, clan):
    """q = 0: every locus of a simulation carries the same label, so m_s is L times 0, 1, 2 or 4 and g_s = [n1_s > 0]."""
    (ind, fa, mo), order = clan
    pro, L, S = order[:20], 130, 16
    r = gen.simuSharing(_ped(gen, ind, fa, mo), pro, loci=L, probRecomb=0.0, simulNo=S, seed=3, labels=True)
    assert r.q == 0 and np.all(r.labels == r.labels[..., :1])
    _same(r.sums[..., 4], r.sums[..., 5])
    assert np.all(r.sums[..., 0] % L == 0) and np.all(r.sums[..., 1] % (L * L) == 0) and np.all(r.sums[..., 2] == L * r.sums[..., 5])
    one = gen.simuSharing(_ped(gen, ind, fa, mo), pro, loci=L, probRecomb=0.0, simulNo=1, seed=3)
    assert set((one.sums[..., 0] // L).ravel().tolist()) <= {0, 1, 2, 4}
    _same(r.sums, sums_of(LinkVector(ind, fa, mo, pro).labels(S, L, 0, 3)))


def test_diagonal(gen, clan):
    (ind, fa, mo), order = clan
    pro, L, S = order[:35], 191, 5
    r = gen.simuSharing(_ped(gen, ind, fa, mo), pro, loci=L, probRecomb=0.05, simulNo=S, seed=6)
    k = np.arange(35)
    assert np.all(r.sums[k, k, 2] == S * L) and np.all(r.sums[k, k, 3] == S * L) and np.all(r.sums[k, k, 4] == S) and np.all(r.sums[k, k, 5] == S)
    assert np.all(r.sums[k, k, 0] >= 2 * S * L) and np.all(r.inbreeding >= 0.0) and np.any(r.inbreeding > 0.0)
    assert np.all(r.segments[k, k] == 1.0) and np.all(r.segment_loci[k, k] == L) and np.all(r.ibd1[k, k] == 1.0)


def test_long_segments_across_word_borders(gen):
    """A parent and its child at q = 1 and L = 4096: the child shares one allele with the parent at every locus, one segment of 64
    words; two sibs share in few, long segments.  A run count that lost the carry between words would see a segment per word."""
    ind = np.arange(1, 6, dtype=np.int64)
    fa = np.array([0, 0, 1, 1, 0], dtype=np.int64)
    mo = np.array([0, 0, 2, 2, 0], dtype=np.int64)
    S, L = 4, 4096
    want = LinkVector(ind, fa, mo, ind).labels(S, L, 1, 12)
    _check(gen, (ind, fa, mo), ind, L, 1, S, 12, want=want)
    s = sums_of(want)
    assert s[0, 2].tolist() == [S * L, S * L * L, S * L, 0, S, S] and s[0, 4].tolist() == [0] * 6
    assert 0 < s[2, 3, 4] <= 3 * S and s[2, 3, 2] > 64 * s[2, 3, 4]                       # sibs: segments longer than a word


def test_simuSharing_meets_the_exact_kinship_on_geneaJi(gen):
    """One condition, not a measurement: |kinship - exact kinship| <= 5 / sqrt(S) for every pair (the mean of S values in [0, 1] has a
    standard deviation of at most 0.5 / sqrt(S), so this is ten of them).  25 and 26 are founders and the parents of 18 and 27: the
    child 18 shares exactly one allele with its father 25 at every locus of every simulation, so that pair's realised kinship never
    varies; the sibs 18 and 27 share now more, now less."""
    ped = gen.genealogy(gen.geneaJi)
    S = 5000
    pro = np.concatenate([gen.pro(ped), [25, 18, 27, 26]]).astype(np.int64)
    r = gen.simuSharing(ped, pro, loci=128, probRecomb=64 / 65536, simulNo=S, seed=7)
    assert r.q == 64
    exact = ExactKinship(*_args(ped)).float64(pro)
    dev = np.abs(r.kinship - exact).max() * np.sqrt(S)
    print("geneaJi, S = %d, L = 128, q = 64, seed 7: largest |kinship - exact kinship| = %.3f / sqrt(S)" % (S, dev))
    assert dev <= 5.0
    assert np.array_equal(r.kinship, r.kinship.T) and r.kinship_sd.shape == (7, 7)
    assert r.kinship_sd[3, 4] == 0.0 and r.kinship[3, 4] == 0.25 and r.kinship_sd[4, 5] > 0.0
    f_exact = 2.0 * np.diag(exact) - 1.0
    assert np.abs(r.inbreeding - f_exact).max() * np.sqrt(S) <= 5.0                       # (the autozygous share of a chromosome: in [0, 1] too)


def test_labels_that_do_not_fit_are_refused_before_any_launch(gen, ji):
    """3 probands x 2 x 2^24 simulations x 4096 loci x 4 bytes are 1.6 TB of labels: more than the device has, less than the 2^48
    bytes create refuses on the host.  compute says so before it allocates or launches anything, and the handle stays usable."""
    ped, pro = ji
    h = gen.SharingPlan(*_args(ped), pro, loci=4096, q=64, simul_no=1 << 24, seed=1, labels=True)
    try:
        with pytest.raises(MemoryError, match="do not fit"):
            h.compute()
        with pytest.raises(ValueError, match="nothing computed"):
            h.sums_to_host()
        assert h.stats()["pair_ms"] == 0.0
    finally:
        h.close()


def test_labels_to_host_without_the_flag(gen, ji):
    ped, pro = ji
    h = gen.SharingPlan(*_args(ped), pro, loci=64, q=64, simul_no=4, seed=1)
    try:
        h.compute()
        with pytest.raises(ValueError, match="GENPHI_LINK_FLAG_LABELS"):
            h.labels_to_host()
        rc = gen._capi.lib().genphi_link_labels_to_host(h._h, None)
        assert rc == gen._capi.GENPHI_ERR_ARG
        assert np.all(h.sums_to_host()[[0, 1, 2], [0, 1, 2], 2] == 4 * 64)
    finally:
        h.close()
