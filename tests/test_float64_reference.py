"""The oracle's Float64 mode (Pedigree.phi64 / phi_rows64: the level sweep with Float64 level matrices) against exact
kinships (tests/exact_kinship.py: Python integers scaled by 2^S) and against the reference's pairwise recursion.  CPU only:
these pin the yardstick that tests/test_float64_parity.py holds the GPU's Float64 sweep to."""
import json
import os

import numpy as np
import pytest

from exact_kinship import ExactKinship, level_steps, max_rel_err, rel_err_bound

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "reference_pinned.json")))


def _bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    if not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{len(bad)} entries differ; first {bad[0]}: {a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}")


def test_exact_reference_reproduces_the_reference_pins(oracle):
    g = GOLD["geneaJi"]
    ind, fa, mo, _ = oracle.read_tsv(os.path.join(HERE, "..", "genlib.jl_amd", "data", "geneaJi.csv"))
    ex = ExactKinship(ind, fa, mo)
    assert ex.pairs64([1], [2])[0] == g["phi_pair_1_2"]                     # test/runtests.jl:49
    pos = {int(x): k for k, x in enumerate(ind)}
    f = lambda x: ex.pairs64([fa[pos[x]]], [mo[pos[x]]])[0] if fa[pos[x]] and mo[pos[x]] else 0.0
    assert f(1) == g["f_1"] and f(17) == g["f_17"]                          # :47-48
    assert np.array_equal(ex.float64(g["pro"]), np.array(g["phi"]))          # :50-52 (exact dyadic rationals)
    assert ex.pairs64([17], [19])[0] == g["phi_pair_founders_17_19"]        # :58-60


def test_phi64_is_exact_on_shallow_pedigrees(oracle):
    """Shallow pedigrees: every kinship and every partial sum is a dyadic rational that Float64 holds exactly, so the
    Float64 sweep must equal the exact kinships bit for bit -- and the reference's Float64 pairwise recursion."""
    from genlib_jl_amd import synth
    ind, fa, mo, _ = oracle.read_tsv(os.path.join(HERE, "..", "genlib.jl_amd", "data", "geneaJi.csv"))
    op = oracle.Pedigree(ind, fa, mo)
    every = op.ind
    m = op.phi64(every)
    _bits_equal(m, ExactKinship(ind, fa, mo).float64(every))
    for a, x in enumerate(every):
        for b, y in enumerate(every):
            assert m[a, b] == op.phi_pair(int(x), int(y)), (x, y)
    assert np.array_equal(op.phi64(GOLD["geneaJi"]["pro"]), np.array(GOLD["geneaJi"]["phi"]))
    for n_ind, n_pro, n_gen, skip, seed in ((1500, 150, 12, 50, 3), (2000, 120, 20, 100, 4), (900, 300, 6, 0, 5)):
        ind, fa, mo, _, pro = synth.random_mating(n_ind, n_pro, n_gen, seed=seed, skip_permille=skip)
        op = oracle.Pedigree(ind, fa, mo)
        ex = ExactKinship(ind, fa, mo)
        m = op.phi64(pro)
        _bits_equal(m, ex.float64(pro))
        assert np.count_nonzero(m) > n_pro
        rows = np.array([0, 7, n_pro - 1])
        _bits_equal(op.phi_rows64(pro, rows), m[rows])


def test_phi64_matches_the_pairwise_recursion_on_genea140_samples(oracle, gen):
    op = oracle.Pedigree.from_file(gen.genea140)
    pro = op.pro()
    rng = np.random.default_rng(140)
    rows = np.unique(np.concatenate([[0, 139], rng.integers(0, 140, 4)]))
    m = op.phi_rows64(pro, rows)
    for q, r in enumerate(rows):
        for c in list(rng.integers(0, 140, 5)) + [r]:
            assert m[q, c] == op.phi_pair(int(pro[r]), int(pro[c])), (r, c)


@pytest.mark.parametrize("n_gen,per_gen", [(60, 15), (120, 12), (200, 10)])
def test_phi64_within_the_rounding_bound_on_deep_pedigrees(oracle, n_gen, per_gen):
    """Deep inbred pedigrees: kinships need more than 53 bits, and the sweep rounds.  Each entry is a sum of non-negative
    terms that picks up at most two roundings per level step along any path, and the scalings are exact: relative error
    <= 2 L 2^-53, L = number of level steps.  Also asserts that many entries really are inexact (the bound has teeth)."""
    from genlib_jl_amd import synth
    ind, fa, mo, _, pro = synth.deep_inbred(n_gen, per_gen, 3)
    op = oracle.Pedigree(ind, fa, mo)
    ex = ExactKinship(ind, fa, mo)
    m = op.phi64(pro)
    L = level_steps(op, pro)
    err = max_rel_err(m, ex.scaled(pro, pro), ex.S)
    inexact = np.count_nonzero(m != ex.float64(pro))
    print(f"deep_inbred({n_gen}, {per_gen}): L = {L}, max relative error {err:.3e} = {err / 2.0 ** -53:.2f} x 2^-53 "
          f"(bound {rel_err_bound(L):.3e}), {inexact} of {m.size} entries not the correctly rounded kinship")
    assert err <= rel_err_bound(L)
    assert inexact >= m.size // 20
    # the upper levels too: a mid-pedigree generation as probands
    mid = ind[(n_gen // 2) * per_gen:(n_gen // 2 + 1) * per_gen]
    assert max_rel_err(op.phi64(mid), ex.scaled(mid, mid), ex.S) <= rel_err_bound(level_steps(op, mid))


@pytest.mark.parametrize("depth", [505, 511, 512, 520, 536, 537, 540])
def test_phi64_float64_subnormals(oracle, depth):
    """Two single-parent lines of `depth` generations below one founder couple: the kinship of their tips is a power of two
    that crosses 2^-1022 (Float64 subnormal) and then underflows to 0 -- no flush to zero before that, and every value
    exact (halving a power of two is exact down to 2^-1074)."""
    from genlib_jl_amd import synth
    ind, fa, mo, _, pro = synth.chain_two_lines(depth)
    op = oracle.Pedigree(ind, fa, mo)
    ex = ExactKinship(ind, fa, mo)
    m = op.phi64(pro)
    _bits_equal(m, ex.float64(pro))
    k = m[0, 1]
    assert k == np.ldexp(1.0, -2 * depth)                                   # 2^-(2 depth): subnormal from depth 512, 0 from 538
    assert (k < np.finfo(np.float64).tiny) == (depth >= 512) and (k > 0) == (depth <= 537)
