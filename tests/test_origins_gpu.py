"""gen.simuOrigins on the MI355X (gen.OriginsPlan, gen.simuOrigins) against the reference of tests/origins_oracle.py: every comparison
of tables is np.array_equal, every handle is computed twice with equal bytes.  Shapes are the smallest at which each part of
csrc/origin.hip can go wrong: word and pair edges of the simulations, forced and ragged panels, forced and ragged label chunks at 1, 2,
7 and 32 groups, allele tables one label short of, at and one label past a multiple of the chunk, group sizes around the number of
waves of the count kernel and its unrolling, empty groups, a hub couple whose 300 children all add into the same four counters, one
selfed founder with 32,767 children in one group (both counter fields near their ends, sums past 2^32), the table by proband on and
off, and the invariants of the definition against gen.CarriersPlan and gen.IdentityPlan in the same process.  A reference is computed
once per pedigree at the largest S and cut to the columns a case needs."""
import os

import numpy as np
import pytest

from origins_oracle import OriginVector, check_invariants, exact_kinship, expected_frequency, pair_index
from random_pedigree import random_pedigree
from test_carriers_gpu import _big_pedigree, _founders_and_sibships

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = [1, 63, 64, 65, 127, 128, 129, 200, 5000]
WAVES = 16                                   # the count kernel's workgroup: 1,024 threads
UNROLL = 4                                   # the individuals a wave has in flight


def _args(ped):
    return ped.ind, ped.father, ped.mother


def _ped(gen, ind, fa, mo):
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b), (np.argwhere(a != b)[:5], a[a != b][:5], b[a != b][:5])


def _rule(n_labels, G, arg):
    """(chunk_labels, chunks, lds_bytes) as the definition states them: the widest chunk is the largest LC with 256 ((LC G) | 1) <=
    163,840, which is also the default."""
    widest = max(lc for lc in range(1, 640) if 256 * ((lc * G) | 1) <= 163840)
    lc = min(n_labels, widest, arg if arg else widest)
    return lc, -(-n_labels // lc), 256 * ((lc * G) | 1)


def _tables(h):
    return h.copies_to_host(), h.autozygous_to_host(), h.matches_to_host(), h.by_proband_to_host() if h.by_proband else None


def _check(gen, args, pro, groups, G, S, seed, ref=None, by_proband=True, **kw):
    """The tables of one handle, computed twice, against the reference; the invariants on the device's tables; returns stats()."""
    if ref is None:
        ref = OriginVector(*args, pro, groups, G, S, seed)
    want = ref.at(S)
    h = gen.OriginsPlan(*args, pro, groups, n_groups=G, simul_no=S, seed=seed, by_proband=by_proband, **kw)
    try:
        _same(h.alleles(), ref.alleles)
        assert (h.n_grouped, h.n_groups) == (ref.n, G)
        for _ in range(2):
            h.compute()
            got = _tables(h)
            for g, w in zip(got, want):
                if g is not None:
                    _same(g, w)
        check_invariants(*got, ref.sizes, S, h.alleles(), ref.pro, ref.group)
        st = h.stats()
        assert st["sweep_ms"] >= 0.0 and st["count_ms"] > 0.0 and st["planes"] == h.planes and (st["n_groups"], st["n"]) == (G, ref.n)
        assert (st["chunk_labels"], st["chunks"], st["lds_bytes"]) == _rule(h.n_labels, G, kw.get("chunk_labels", 0))
        cols = kw.get("panel_cols", 0)
        pairs = min(-(-S // 128), -(-cols // 128)) if cols else -(-S // 128)
        assert (st["panel_cols"], st["panels"]) == (128 * pairs, -(-(-(-S // 128)) // pairs))
        assert st["count_bytes"] == 2 * ref.n * h.planes * 16 * -(-S // 128) * st["chunks"]
        assert st["algorithmic_bytes"] == 48 * h.planes * (2 * h.n_live - h.n_labels) * -(-S // 128)
        return st
    finally:
        h.close()


@pytest.fixture(scope="module")
def ji(gen):
    ped = gen.genealogy(gen.geneaJi)
    pro = gen.pro(ped)
    groups = np.array([0, 0, 1], dtype=np.int32)
    assert len(pro) == 3
    return ped, pro, groups, OriginVector(*_args(ped), pro, groups, 2, 5000, 2024)


def _big_groups(pro):
    """Three groups over the 40 listed probands of the big case (38 distinct: 0, 17 and 33 are one proband) and four of them in none."""
    groups = (np.arange(len(pro)) % 3).astype(np.int32)
    groups[[17, 33]] = groups[0]
    groups[[2, 11, 20, 29]] = -1
    return groups


@pytest.fixture(scope="module")
def big():
    """The reference of the 600-individual case at S = 5000 in three groups."""
    args, pro, _ = _big_pedigree()
    groups = _big_groups(pro)
    return args, pro, groups, OriginVector(*args, pro, groups, 3, 5000, 9)


@pytest.mark.parametrize("S", EDGES)
def test_word_and_pair_edges(gen, ji, S):
    ped, pro, groups, ref = ji
    st = _check(gen, _args(ped), pro, groups, 2, S, 2024, ref=ref)
    assert st["panels"] == 1 and st["chunks"] == 1


def test_big_case_has_the_shapes_it_claims(big):
    (ind, fa, mo), pro, groups, ref = big
    o = ref.o
    assert o.levels >= 5 and o.n_live >= 150 and o.planes >= 6 and o.n_labels > 64
    assert ref.n == 34 and ref.sizes.tolist() == [13, 13, 8] and np.sum(groups == -1) == 4
    assert fa[ind == pro[5]][0] == 0 and mo[ind == pro[5]][0] == 0 and groups[5] >= 0 and np.isin(pro[8], np.union1d(fa, mo)) and groups[8] >= 0
    copies, autozygous, matches, by_pro = ref.at(5000)
    assert autozygous.any() and all(matches[p].any() for p in range(6)) and by_pro.max() > 0


def test_forced_panels(gen, big):
    args, pro, groups, ref = big
    for cols, panels in ((128, 40), (1000, 5), (5000, 1), (0, 1)):
        st = _check(gen, args, pro, groups, 3, 5000, 9, ref=ref, panel_cols=cols)
        assert st["panels"] == panels


@pytest.mark.parametrize("G", [1, 2, 7, 32])
def test_forced_chunks(gen, big, G):
    """One chunk, several chunks and a ragged last chunk at 1, 2, 7 and 32 groups (the widest chunk is 639, 319, 91 and 19 labels);
    then ragged panels and ragged chunks at once."""
    args, pro, _, three = big
    n = three.n_labels
    groups = (np.arange(len(pro)) % G).astype(np.int32)
    groups[[17, 33]] = groups[0]
    groups[[2, 11]] = -1
    ref = OriginVector(*args, pro, groups, G, 1000, 9)
    widest = 639 // G
    st = _check(gen, args, pro, groups, G, 1000, 9, ref=ref)
    assert st["chunk_labels"] == min(n, widest) and st["chunks"] == -(-n // widest)
    if n <= widest:
        assert _check(gen, args, pro, groups, G, 1000, 9, ref=ref, chunk_labels=n)["chunks"] == 1
    for lc in (6, 16):
        assert n % lc != 0, "the last chunk is not ragged"
        st = _check(gen, args, pro, groups, G, 1000, 9, ref=ref, chunk_labels=lc)
        assert st["chunk_labels"] == lc and st["chunks"] == -(-n // lc) >= 2
    st = _check(gen, args, pro, groups, G, 1000, 9, ref=ref, chunk_labels=9, panel_cols=384)
    assert st["panels"] == 3 and 8 % 3 != 0 and st["chunks"] >= 2


@pytest.mark.parametrize("G,lc", [(1, 32), (2, 32), (7, 32), (32, 16)])
@pytest.mark.parametrize("n_full,n_half", [(31, 1), (32, 0), (31, 3)])
def test_allele_tables_around_a_multiple_of_the_chunk(gen, n_full, n_half, G, lc):
    """63, 64 and 65 labels in chunks of 32 (of 16 at 32 groups): one label short of a whole number of chunks, exactly that, and one
    label past it.  Everyone is listed, in the groups 0, 1, .., G - 1, 0, .."""
    ind, fa, mo = _founders_and_sibships(n_full, n_half)
    n_labels = 2 * n_full + n_half
    groups = (np.arange(len(ind)) % G).astype(np.int32)
    ref = OriginVector(ind, fa, mo, ind, groups, G, 200, 3)
    assert ref.n_labels == n_labels and n_labels in (63, 64, 65)
    st = _check(gen, (ind, fa, mo), ind, groups, G, 200, 3, ref=ref, chunk_labels=lc)
    assert (st["chunk_labels"], st["chunks"]) == (lc, -(-n_labels // lc))
    assert _check(gen, (ind, fa, mo), ind, groups, G, 200, 3, ref=ref)["chunks"] == -(-n_labels // (639 // G))


@pytest.fixture(scope="module")
def clan():
    """200 individuals in few generations, closely related: the pool the group-size tests draw from."""
    rng = np.random.default_rng(3)
    ind, fa, mo, _ = random_pedigree(rng, 200, p_founder=0.1, p_one_parent=0.05, p_selfing=0.05, max_back=20)
    return (ind, fa, mo), rng.permutation(ind)


@pytest.mark.parametrize("n", [1, 3, 4, 5, WAVES - 1, WAVES, WAVES + 1, WAVES * UNROLL - 1, WAVES * UNROLL, WAVES * UNROLL + 1])
def test_group_sizes(gen, clan, n):
    """n_a = 1, 3, 4, 5; the number of waves +- 1; the waves times the unrolling +- 1.  Group 1 holds n probands, group 2 three more,
    so the border between the groups in the row list moves across the same edges; group 0 has no listed proband, and the trailing
    groups 3 and 4 are absent; two listed probands are in no group."""
    args, order = clan
    pro = np.concatenate([order[:n], order[150:153], order[160:162]])
    groups = np.concatenate([np.full(n, 1), np.full(3, 2), np.full(2, -1)]).astype(np.int32)
    _check(gen, args, pro, groups, 5, 200, 5)


def test_hub_couple_with_300_children(gen):
    """Every wave adds into the same four labels: k of the father's two alleles is 300 per simulation.  All 300 children in one
    group, then split over two, where the same cells are met from both halves of the row list."""
    ind = np.arange(1, 303, dtype=np.int64)
    fa = np.where(ind > 2, 1, 0).astype(np.int64)
    mo = np.where(ind > 2, 2, 0).astype(np.int64)
    pro = ind[2:]
    one = OriginVector(ind, fa, mo, pro, None, 1, 200, 3)
    copies, autozygous, matches, _ = one.at(200)
    assert copies.tolist() and np.all(copies[0, 0] + copies[0, 1] == 300 * 200) and not autozygous.any()
    st = _check(gen, (ind, fa, mo), pro, None, 1, 200, 3, ref=one)
    assert st["levels"] == 2 and st["planes"] == 2
    groups = (np.arange(300) >= 137).astype(np.int32)
    two = OriginVector(ind, fa, mo, pro, groups, 2, 200, 3)
    _check(gen, (ind, fa, mo), pro, groups, 2, 200, 3, ref=two)
    check_invariants(*two.at(200), two.sizes, 200, merged=one.at(200)[:3])


def test_both_counter_fields_near_their_ends(gen):
    """One founder selfed, 32,769 children, S = 64: group 0 holds 32,767 of them, so c1 of either allele is about 3/4 of them and c2
    about 1/4; group 1 holds the last two.  m_00 of one simulation is near 32,767^2 / 2 = 2^29, and the sum over the 64 lanes of a
    wave passes 2^32: the 64-bit reduce is what is tested."""
    n = 32767
    ind = np.arange(1, n + 4, dtype=np.int64)
    fa = np.where(ind > 1, 1, 0).astype(np.int64)
    mo = fa.copy()
    pro = ind[1:]
    groups = (np.arange(n + 2) >= n).astype(np.int32)
    ref = OriginVector(ind, fa, mo, pro, groups, 2, 64, 11)
    copies, autozygous, matches, by_pro = ref.at(64)
    assert ref.sizes.tolist() == [n, 2] and copies[0].min() > 64 * 16384 + 64 * 4096 and autozygous[0].min() > 64 * 4096
    assert matches[0].min() > 2**32 and matches[1].min() > 0
    st = _check(gen, (ind, fa, mo), pro, groups, 2, 64, 11, ref=ref)
    assert (st["n"], st["planes"], st["chunks"]) == (n + 2, 1, 1)


def test_by_proband_on_and_off(gen, big):
    """Invariant 7: the other three tables hold the same bytes with and without autozygous_pro."""
    args, pro, groups, ref = big
    on = gen.OriginsPlan(*args, pro, groups, n_groups=3, simul_no=1000, seed=9, by_proband=True, chunk_labels=16)
    off = gen.OriginsPlan(*args, pro, groups, n_groups=3, simul_no=1000, seed=9, by_proband=False, panel_cols=256)
    try:
        on.compute()
        off.compute()
        a, b = _tables(on), _tables(off)
        assert b[3] is None
        check_invariants(*a, ref.sizes, 1000, other=b)
        for g, w in zip(a, ref.at(1000)):
            _same(g, w)
        with pytest.raises(ValueError, match="without by_proband"):
            off.by_proband_to_host()
    finally:
        on.close()
        off.close()


def test_against_the_carriers_and_the_identity_states(gen, big):
    """Invariants 2 and 3, every handle on the device in this process.  2: one group, against gen.CarriersPlan with no controls and
    every column.  3: against gen.IdentityPlan on the distinct grouped probands, the numerator of its kinship pair by pair."""
    args, pro, groups, ref = big
    S, seed = 777, 12345678901234567
    one = gen.OriginsPlan(*args, pro, simul_no=S, seed=seed, panel_cols=256)
    carry = gen.CarriersPlan(*args, pro, simul_no=S, seed=seed)
    three = gen.OriginsPlan(*args, pro, groups, n_groups=3, simul_no=S, seed=seed, chunk_labels=16)
    ident = gen.IdentityPlan(*args, ref.pro, simul_no=S, seed=seed)
    try:
        for h in (one, carry, three, ident):
            h.compute()
        _same(one.alleles(), carry.alleles())
        carriers, homozygotes = carry.carriers_to_host().astype(np.int64), carry.homozygotes_to_host().astype(np.int64)
        assert carriers.shape[1] == one.n_grouped + 1
        weight = np.arange(carriers.shape[1], dtype=np.int64)
        _same(one.copies_to_host()[0], (carriers + homozygotes) @ weight)                              # 2
        _same(one.autozygous_to_host()[0], homozygotes @ weight)
        c = ident.counts_to_host().astype(np.int64)                                                    # 3
        num = 4 * c[..., 0] + 2 * (c[..., 2] + c[..., 4] + c[..., 6]) + c[..., 7]
        copies, autozygous, matches, _ = _tables(three)
        whole = 0
        for a in range(3):
            ia = np.flatnonzero(ref.group == a)
            assert autozygous[a].sum() == c[ia, ia, 0].sum()
            for b in range(a, 3):
                ib = np.flatnonzero(ref.group == b)
                block = num[np.ix_(ia, ib)]
                want = np.triu(block, 1).sum() if a == b else block.sum()
                assert matches[pair_index(a, b, 3)].sum() == want > 0
                whole += want
        everyone = gen.OriginsPlan(*args, pro, np.where(groups >= 0, 0, -1), simul_no=S, seed=seed)    # 4: the three groups merged, the same list
        try:
            everyone.compute()
            assert everyone.matches_to_host().sum() == whole == np.triu(num, 1).sum()
            check_invariants(copies, autozygous, matches, None, ref.sizes, S, merged=_tables(everyone)[:3])
        finally:
            everyone.close()
    finally:
        for h in (one, carry, three, ident):
            h.close()


def test_order_repeats_renumbering_branching_and_seeds(gen, big):
    """Invariant 7 through gen.simuOrigins: the order and the repeats of the list change no byte, renumbering the groups permutes the
    tables; gen.branching first changes nothing; fresh seeds differ and replay."""
    (ind, fa, mo), pro, groups, ref = big
    ped = _ped(gen, ind, fa, mo)
    S = 1000
    names = ["b", "c", "a"]                                                           # group 0 is "b": sorted, it is table row 1
    of = {int(p): names[g] for p, g in zip(pro.tolist(), groups.tolist()) if g >= 0}
    full = gen.simuOrigins(ped, pro, of, simulNo=S, seed=9, byProband=True)
    want = ref.at(S)
    at = [1, 2, 0]                                                                    # the table row of the reference's group a
    assert full.names == ["a", "b", "c"] and full.sizes[at].tolist() == ref.sizes.tolist() and (full.simulNo, full.seed) == (S, 9)
    _same(full.pro, ref.pro)
    _same(full.alleles, ref.alleles)
    _same(full.copies[at], want[0])
    _same(full.autozygous[at], want[1])
    for a in range(3):
        for b in range(a, 3):
            _same(full.matches[at[a], at[b]], want[2][pair_index(a, b, 3)])
            _same(full.matches[at[b], at[a]], want[2][pair_index(a, b, 3)])
    _same(full.autozygous_pro, want[3])
    rng = np.random.default_rng(4)
    order = rng.permutation(len(pro))
    for p in (pro[order], np.concatenate([pro[::-1], pro[:7]])):
        r = gen.simuOrigins(ped, p, of, simulNo=S, seed=9, byProband=True)
        back = np.array([r.pro.tolist().index(q) for q in full.pro.tolist()])
        for g, w in ((r.copies, full.copies), (r.autozygous, full.autozygous), (r.matches, full.matches), (r.autozygous_pro[back], full.autozygous_pro)):
            assert g.tobytes() == w.tobytes()
    pruned = gen.branching(ped, pro=pro)
    assert len(pruned) < len(ped)
    r = gen.simuOrigins(pruned, pro, of, simulNo=S, seed=9)
    _same(r.alleles, full.alleles)
    _same(r.matches, full.matches)
    assert r.autozygous_pro is None
    assert not np.array_equal(gen.simuOrigins(ped, pro, of, simulNo=S, seed=10).copies, full.copies)
    a, b = gen.simuOrigins(ped, pro, of, simulNo=256), gen.simuOrigins(ped, pro, of, simulNo=256)
    assert a.seed != b.seed and not np.array_equal(a.copies, b.copies)                # fresh seeds
    replay = gen.simuOrigins(ped, pro, of, simulNo=256, seed=a.seed)
    _same(replay.copies, a.copies)
    _same(replay.matches, a.matches)
    # the floats are formed from these integers
    assert np.allclose(full.frequency.sum(axis=1), 1.0, atol=1e-12) and np.allclose(full.kinship_by_allele.sum(axis=2), full.kinship, atol=1e-12)
    assert np.allclose(full.partial_inbreeding().sum(axis=1), full.autozygous_pro.sum(axis=1) / float(S), atol=1e-12)
    assert np.allclose(full.inbreeding_by_founder().sum(axis=1), full.inbreeding, atol=1e-12) and np.allclose(full.share.sum(axis=2), 1.0, atol=1e-12)
    top = full.ranking("a", "b", k=5)
    assert len(top) == 5 and np.all(np.diff(full.share[0, 1][top]) <= 0)


def test_statistics_on_geneaJi(gen, ji):
    """S = 5,000, a fixed seed.  The sum over the alleles of the kinship shares is the mean kinship of the pair of groups: within
    5 / sqrt(S) of the exact one, the project's bound for gene dropping.  frequency[a, l] is the mean over the simulations of a
    value in [0, 1], whose standard deviation is at most 0.5: 5 / sqrt(S) is ten standard deviations of that mean.  Both exact values
    come from host recursions (tests/origins_oracle.py); the reference gives the same figures on the CPU for this seed."""
    ped, pro, groups, ref = ji
    S = 5000
    r = gen.simuOrigins(ped, pro, {int(p): "g%d" % g for p, g in zip(pro.tolist(), groups.tolist())}, simulNo=S, seed=2024)
    _same(r.copies, ref.at(S)[0])
    exact = exact_kinship(ref.o, ref.pro, ref.group, 2)
    got = r.kinship_by_allele.sum(axis=2)
    dev = np.abs(got - exact)[[0, 0], [0, 1]].max() * np.sqrt(S)
    print("geneaJi, S = %d: kinship %s, exact %s, the largest deviation is %.3f / sqrt(S)" % (S, got[[0, 0], [0, 1]], exact[[0, 0], [0, 1]], dev))
    assert dev <= 5.0 and np.isnan(exact[1, 1]) and np.isnan(r.kinship[1, 1]) and exact[0, 0] > 0 and exact[0, 1] > 0
    freq = expected_frequency(ref.o, ref.pro, ref.group, 2)
    dev = np.abs(r.frequency - freq).max() * np.sqrt(S)
    print("geneaJi, S = %d: the largest deviation of an allele frequency is %.3f / sqrt(S)" % (S, dev))
    assert dev <= 5.0 and np.allclose(freq.sum(axis=1), 1.0, atol=1e-12)


def test_simuOrigins_on_genea140_with_the_seven_populations(gen):
    ped = gen.genealogy(gen.genea140)
    pop = gen._pop(os.path.join(ROOT, "tests", "golden", "pop140.csv"))
    S = 200
    r = gen.simuOrigins(ped, groups=pop, simulNo=S, seed=21, byProband=True)
    pro = gen.pro(ped)
    names = sorted(set(pop.values()))
    assert r.names == names and len(names) == 7 and r.sizes.sum() == len(r.pro) == 140 and np.array_equal(r.pro, pro)
    groups = np.array([names.index(pop[int(p)]) for p in pro.tolist()], dtype=np.int32)
    ref = OriginVector(*_args(ped), pro, groups, 7, S, 21)
    want = ref.at(S)
    _same(r.copies, want[0])
    _same(r.autozygous, want[1])
    for a in range(7):
        for b in range(a, 7):
            _same(r.matches[a, b], want[2][pair_index(a, b, 7)])
    _same(r.autozygous_pro, want[3])
    h = gen.OriginsPlan(*_args(ped), pro, groups, n_groups=7, simul_no=S, seed=21)
    try:
        st = h.stats()
        assert (st["chunk_labels"], st["chunks"]) == (91, -(-h.n_labels // 91)) and st["chunks"] > 100
    finally:
        h.close()
    kin = r.kinship
    assert np.all(kin >= 0) and np.all(np.diag(kin) >= kin.min()) and r.partial_inbreeding().shape == (140, len(r.founders))
