"""gen.gc on the GPU (csrc/gc.hip) against the oracles of tests/gc_oracle.py: bit for bit against the reference's
literal path sums where those are exact (sweeps of at most 24 steps), against the correctly rounded exact contribution
up to 52 steps, and within 1 Float32 ulp of it beyond."""
import numpy as np
import pytest

from gc_oracle import ExactGC, divergence_pedigree, gc_exact_rows, gc_literal
from test_gc_reference import QUIRK_ANC, QUIRK_EXPECTED, QUIRK_PRO, quirk_pedigree

pytestmark = pytest.mark.gpu


def _ped(gen, ind, fa, mo, sex=None, sort=True):
    sex = np.ones(len(ind), dtype=np.int64) if sex is None else sex
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}, sort=sort)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    bad = np.argwhere(_bits(a) != _bits(b))
    assert len(bad) == 0, f"{len(bad)} entries differ, first at {tuple(bad[0])}: {a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}"


def _one_parent_synth(synth):
    """A random-mating pedigree with parents from two generations back (dragged members) and one-parent members:
    every 13th non-founder loses its mother, every 17th its father."""
    ind, fa, mo, sex, pro = synth.random_mating(4000, 400, 10, skip_permille=50)
    fa, mo = fa.copy(), mo.copy()
    k = np.arange(len(ind))
    mo[(k % 13 == 5) & (fa != 0)] = 0
    fa[(k % 17 == 3) & (mo != 0)] = 0
    return ind, fa, mo, sex, pro


@pytest.fixture(scope="module")
def genea140(gen):
    ped = gen.genealogy(gen.genea140)
    return ped, gen.pro(ped), gen.founder(ped)


@pytest.fixture(scope="module")
def genea140_literal(genea140):
    ped, pro, anc = genea140
    return gc_literal(ped.ind, ped.father, ped.mother, pro, anc)


def test_geneaJi_default_arguments(gen):
    ped = gen.genealogy(gen.geneaJi)
    out = gen.gc(ped)
    _same(out, gc_literal(ped.ind, ped.father, ped.mother, gen.pro(ped), gen.founder(ped)))


def test_genea140_default_arguments(gen, genea140, genea140_literal):
    ped, _, _ = genea140
    out = gen.gc(ped)
    _same(out, genea140_literal)
    assert float(np.sum(out, dtype=np.float64)) == 140.0               # test/runtests.jl:28


@pytest.mark.parametrize("panel", [1, 3, 64])
def test_genea140_column_panels(gen, genea140, genea140_literal, monkeypatch, panel):
    """7,399 founders in panels of 1, 3 (a ragged last panel of 1) and 64 (ragged: 39) columns."""
    monkeypatch.setenv("GENPHI_GC_PANEL", str(panel))
    ped, pro, anc = genea140
    h = gen.GCPlan(ped.ind, ped.father, ped.mother, pro, anc)
    try:
        h.compute()
        assert h.stats()["panel_cols"] == panel
        _same(h.result_to_host(), genea140_literal)
    finally:
        h.close()


def test_hand_built_quirks(gen):
    ped = quirk_pedigree(gen)
    _same(gen.gc(ped, pro=QUIRK_PRO, ancestors=QUIRK_ANC), QUIRK_EXPECTED)


def _mixed_lists(ped, gen, rng, n_anc):
    """Unsorted, duplicated, non-leaf and founder probands; a few ancestors with non-founders, duplicates, an unrelated
    founder and a proband among them."""
    leaves = gen.pro(ped)
    founders = gen.founder(ped)
    nonleaf = np.setdiff1d(ped.ind, leaves)
    pro = np.concatenate([rng.choice(leaves, 40, replace=False), rng.choice(nonleaf, 6, replace=False),
                          rng.choice(founders, 3, replace=False)])
    pro = np.concatenate([pro, pro[[0, 7, 41]]])                      # repeats: a leaf, a leaf, a non-leaf
    rng.shuffle(pro)
    unrelated = [f for f in founders if f in set(leaves.tolist())]        # a founder without children
    anc = list(rng.choice(founders, n_anc - 9, replace=False)) + list(rng.choice(nonleaf, 3, replace=False))
    anc += [anc[0], anc[-1], int(pro[2])]                                 # duplicated founder, duplicated non-founder, a proband
    anc += [int(unrelated[0])] if unrelated else [int(founders[-1])]
    anc += [int(leaves[0]), int(pro[5])]
    assert len(anc) == n_anc
    return pro.astype(np.int64), np.asarray(anc, dtype=np.int64)


@pytest.mark.parametrize("n_anc", [13, 63])
def test_genea140_mixed_lists(gen, genea140, n_anc):
    ped, _, _ = genea140
    pro, anc = _mixed_lists(ped, gen, np.random.default_rng(n_anc), n_anc)
    _same(gen.gc(ped, pro=pro, ancestors=anc), gc_literal(ped.ind, ped.father, ped.mother, pro, anc))


def test_one_parent_synthetic_mixed_lists(gen, synth_one_parent):
    ped = synth_one_parent
    pro, anc = _mixed_lists(ped, gen, np.random.default_rng(5), 21)
    out = gen.gc(ped, pro=pro, ancestors=anc)
    _same(out, gc_literal(ped.ind, ped.father, ped.mother, pro, anc))
    _same(out, gc_exact_rows(ped.ind, ped.father, ped.mother, pro, anc))


@pytest.fixture(scope="module")
def synth_one_parent(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, _ = _one_parent_synth(synth)
    return _ped(gen, ind, fa, mo, sex)


def test_one_parent_synthetic_all_founders(gen, synth_one_parent):
    ped = synth_one_parent
    pro, anc = gen.pro(ped), gen.founder(ped)
    out = gen.gc(ped)
    _same(out, gc_exact_rows(ped.ind, ped.father, ped.mother, pro, anc))
    # one-parent members pass on half: rows of leaves with a lost parent sum to less than 1
    assert np.all(out.sum(axis=1, dtype=np.float64) <= 1.0) and np.any(out.sum(axis=1, dtype=np.float64) < 1.0)


def test_unsorted_ranks(gen):
    """sort=false: ranks follow a parents-first file order, not the depth."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, _ = _one_parent_synth(synth)
    ind, fa, mo, sex = synth.parents_first_shuffle(ind, fa, mo, sex, seed=3)
    ped = _ped(gen, ind, fa, mo, sex, sort=False)
    assert not np.array_equal(ped.ind, _ped(gen, ind, fa, mo, sex).ind)
    pro, anc = _mixed_lists(ped, gen, np.random.default_rng(9), 17)
    _same(gen.gc(ped, pro=pro, ancestors=anc), gc_literal(ped.ind, ped.father, ped.mother, pro, anc))
    _same(gen.gc(ped), gc_exact_rows(ped.ind, ped.father, ped.mother, gen.pro(ped), gen.founder(ped)))


def test_probands_all_founders(gen, synth_one_parent):
    """Zero level steps: only founders among the probands (leaves and parents)."""
    ped = synth_one_parent
    founders = gen.founder(ped)
    leaves = set(gen.pro(ped).tolist())
    lone = [f for f in founders if f in leaves]
    pro = np.asarray(lone[:3] + list(founders[:5]) + lone[:1], dtype=np.int64)
    anc = np.asarray(list(founders[:4]) + lone[:2] + lone[1:2], dtype=np.int64)
    out = gen.gc(ped, pro=pro, ancestors=anc)
    _same(out, gc_literal(ped.ind, ped.father, ped.mother, pro, anc))
    assert len(lone) >= 3 and out.sum(dtype=np.float64) >= 3.0      # lone[0] once, lone[1] in two columns


def test_empty_lists(gen, genea140):
    ped, pro, anc = genea140
    assert gen.gc(ped, pro=[], ancestors=anc[:5]).shape == (0, 5)
    assert gen.gc(ped, pro=pro[:4], ancestors=[]).shape == (4, 0)
    assert gen.gc(ped, pro=[], ancestors=[]).shape == (0, 0)


def test_deep_inbred_correctly_rounded(gen):
    """40 generations: 39 steps, more than Float32 path sums hold exactly, fewer than Float64's 52."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.deep_inbred(40, 50, 3)
    ped = _ped(gen, ind, fa, mo, sex)
    anc = gen.founder(ped)
    out = gen.gc(ped, pro=pro, ancestors=anc)
    _same(out, gc_exact_rows(ped.ind, ped.father, ped.mother, pro, anc))


def test_deep_inbred_200_generations_within_one_ulp(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.deep_inbred(200, 50, 3)
    ped = _ped(gen, ind, fa, mo, sex)
    anc = np.concatenate([gen.founder(ped), ped.ind[[2000, 5001, 9000]]])
    out = gen.gc(ped, pro=pro, ancestors=anc)
    ref = gc_exact_rows(ped.ind, ped.father, ped.mother, pro, anc)
    assert np.count_nonzero(ref) > len(pro)
    gap = np.abs(out.astype(np.float64) - ref.astype(np.float64))
    assert np.all(gap <= np.spacing(np.abs(ref)).astype(np.float64)), float(np.max(gap / np.spacing(np.abs(ref))))


def test_divergence_pedigree_correctly_rounded(gen):
    """Where the reference's Float32 path sums lose 128 small terms (test_gc_reference.py), gen.gc returns the exact value."""
    ind, fa, mo, sex, P, A = divergence_pedigree()
    ped = _ped(gen, ind, fa, mo, sex)
    out = gen.gc(ped, pro=[P], ancestors=[A, A])
    assert out[0, 0] == np.float32(0.25 + 2.0 ** -23) and out[0, 1] == out[0, 0]
    assert gc_literal(ped.ind, ped.father, ped.mother, [P], [A])[0, 0] == np.float32(0.25)


def test_cfg3_all_founders(gen):
    """cfg3: 1e4 probands x 6,633 founders (265 MB).  19 steps: every entry a multiple of 2^-19, every row a partition of
    the proband's genome (sums to 1 exactly), 64 sampled rows equal to the exact ones."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(100_000, 10_000, 20)
    ped = _ped(gen, ind, fa, mo, sex)
    anc = gen.founder(ped)
    assert len(anc) == 6633
    out = gen.gc(ped, pro=pro, ancestors=anc)
    assert out.shape == (10_000, 6633)
    scaled = out.astype(np.float64) * 2.0 ** 19
    assert np.array_equal(scaled, np.floor(scaled))
    assert np.all(out.sum(axis=1, dtype=np.float64) == 1.0)
    sample = np.random.default_rng(3).choice(len(pro), 64, replace=False)
    _same(out[sample], gc_exact_rows(ped.ind, ped.father, ped.mother, pro, anc, sample=sample))
