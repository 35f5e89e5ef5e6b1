"""The second CPU restatement of sparse_phi (oracle/slot_oracle.cpp: a dense matrix of the live set, slots reused) against the literal
one (oracle/sparse_oracle.cpp: the reference's dictionaries), on every sparse_phi case the suite uses and on all of genea140: every
getindex, `show`, both Float64 sums and the stored entries.  This is what lets the slot oracle stand in for the literal one at
widths where the dictionaries cannot run (tests/test_sparse_phi_wide.py).  No GPU."""
import numpy as np

import wide_waves as W


def _lexsorted(r, c, v):
    o = np.lexsort((v, c, r))
    return r[o], c[o], v[o]


def _same(oracle, ind, fa, mo, pro, sort=True):
    ped = oracle.Pedigree(ind, fa, mo, sort=sort)
    want = oracle.SparsePhi(ped, pro)
    got = oracle.SlotSparsePhi(ped, pro)
    ids = got.ids
    ref = np.array([[want[(x, y)] for y in ids] for x in ids], dtype=np.float32)
    assert np.array_equal(got.matrix(), ref)
    nr, nz, sa, sd = got.info()
    wr, wz, wa, wd = want.info()
    assert (nr, nz) == (wr, wz), ((nr, nz), (wr, wz))
    assert abs(sa - wa) <= 1e-12 * max(1.0, abs(wa)) and abs(sd - wd) <= 1e-12 * max(1.0, abs(wd)), ((sa, sd), (wa, wd))
    assert got.show() == want.show()
    if nr > 1:
        assert got.phi_mean() == want.phi_mean()
    for a, b in zip(_lexsorted(*got.entries()), _lexsorted(*want.entries())):
        assert np.array_equal(a, b)
    return got, want


def test_slot_oracle_equals_the_dictionary_oracle(gen, oracle):
    from genlib_jl_amd import synth
    oj = oracle.read_tsv(gen.geneaJi)
    got, _ = _same(oracle, *oj[:3], [1, 2, 29])
    assert got.show() == "3×3 KinshipMatrix with 6 stored entries." and got[1, 2] == 0.37109375       # test/runtests.jl:55-57
    assert float(got.phi_mean()) == 0.171875
    _same(oracle, *oj[:3], [29, 1, 9, 1, 17])                               # an ancestor and a founder among the probands, a duplicate
    for args, kw, seed in [((600, 60, 6), dict(skip_permille=100), 1), ((2000, 150, 8), dict(skip_permille=0), 2),
                           ((1500, 100, 12), dict(skip_permille=200, seed=9), 3)]:
        ind, fa, mo, sex, pro = synth.random_mating(*args, **kw)
        perm = np.random.default_rng(seed).permutation(len(ind))
        _same(oracle, ind[perm], fa[perm], mo[perm], pro)
        _same(oracle, ind, fa, mo, pro[::3])
    one = synth.random_mating(900, 80, 7, skip_permille=50, seed=3)
    mo1 = one[2].copy(); mo1[::13] = 0                                      # one-parent members
    _same(oracle, one[0], one[1], mo1, one[4])
    # the 8-member example of test_sparse_phi_unsorted_ranks: (6, 5) = 0.125 outlives its column
    ind = np.arange(1, 9)
    fa = np.array([0, 0, 1, 0, 3, 1, 0, 5]); mo = np.array([0, 0, 2, 0, 4, 2, 0, 7])
    got, _ = _same(oracle, ind, fa, mo, [6, 8], sort=False)
    assert got.show() == "2×2 KinshipMatrix with 3 stored entries." and float(got.phi_mean()) == 0.125
    assert got.entries()[2].tolist()[-1] == 0.125
    _same(oracle, ind, fa, mo, [6, 8], sort=True)
    n_cross = 0
    for args, kw, seed in [((600, 60, 6), dict(skip_permille=100), 1), ((2000, 150, 8), dict(skip_permille=0), 2),
                           ((1500, 100, 12), dict(skip_permille=200, seed=9), 3), ((900, 80, 7), dict(skip_permille=50, seed=3), 4)]:
        ind, fa, mo, sex, pro = synth.random_mating(*args, **kw)
        if seed == 4:
            mo = mo.copy(); mo[::13] = 0
        i2, f2, m2, s2 = synth.parents_first_shuffle(ind, fa, mo, sex, seed=seed)
        extra = i2[np.random.default_rng(seed).integers(0, len(i2), 12)]    # ancestors among the probands
        for p in (pro, np.concatenate([pro[::2], extra])):
            a, _ = _same(oracle, i2, f2, m2, p, sort=False)
            b, _ = _same(oracle, i2, f2, m2, p, sort=True)
            n_cross += a.info()[1] != b.info()[1]
    assert n_cross >= 3
    g = oracle.read_tsv(gen.genea140)
    pro140 = gen.pro(gen.genealogy(gen.genea140))
    _same(oracle, *g[:3], pro140[:25])
    _same(oracle, *g[:3], pro140[:25], sort=False)
    g2 = synth.parents_first_shuffle(*g, seed=11)
    _same(oracle, *g2[:3], pro140[5:30], sort=False)
    # the generator of the wide-wave GPU tests, small: skipped generations, one-parent members, early probands, shuffled
    w = W.wide_waves([40, 60, 90, 50, 30], early_probands=[2, 2], skip_permille=100, one_parent_every=7)
    _same(oracle, *w[:3], w[4])
    i2, f2, m2, _ = synth.parents_first_shuffle(*w[:4], seed=2)
    _same(oracle, i2, f2, m2, w[4], sort=False)


def test_slot_oracle_equals_the_dictionary_oracle_on_all_of_genea140(gen, oracle):
    """genea140 with its 140 probands (the bench's sparse140): ~40 s for the dictionaries, ~3 s for the slots on 8 CPUs."""
    g = oracle.read_tsv(gen.genea140)
    got, _ = _same(oracle, *g[:3], gen.pro(gen.genealogy(gen.genea140)))
    assert got.peak_live() > 7000 and got.info()[:2] == (140, 7442)


def test_slot_oracle_rejects_unknown_probands(gen, oracle):
    ped = oracle.Pedigree.from_file(gen.geneaJi)
    try:
        oracle.SlotSparsePhi(ped, [424242])
    except KeyError:
        pass
    else:
        raise AssertionError("unknown proband ID accepted")
    K = oracle.SlotSparsePhi(ped, [1, 2])
    try:
        K.get([1, 2], [2, 17])
    except KeyError:
        pass
    else:
        raise AssertionError("a non-proband ID read")


def test_wide_wave_cases_reach_their_regimes(gen):
    """The wide-wave GPU cases (tests/test_sparse_phi_wide.py), host side only: the schedule gen.sparse_phi follows
    (_capi.sparse_schedule, itself checked against the reference's queue in test_sparse_schedule.py) has the widths each
    case relies on, so a change to the generator or the schedule cannot make a GPU case silently stop reaching its path."""
    for name in W.CASES:
        W.check_regime(gen, name, *W.case(name))
    n_old, n_new = W.waves(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert len(n_old) == 0 and len(n_new) == 0
