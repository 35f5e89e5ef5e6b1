"""GPU parity tests proper: the HIP path (through the C-ABI) against the CPU oracle on the
same inputs -- bit-exact (the north-star tolerance is <= 1e-12 absolute on Float32 results;
we assert exact equality, which implies it) -- plus the committed golden vectors and
size-independent properties at larger sizes."""
import json
import os

import numpy as np
import pytest

from random_pedigree import random_pedigree as _random_pedigree

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "reference_pinned.json")))
TOL = 1e-12   # north_star tolerance; every comparison below is exact, i.e. 0 <= TOL


def _gpu_phi(gen, ind, fa, mo, sex, pro, **kw):
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    return gen.phi(ped, pro, **kw)


def _assert_equal(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{len(bad)} entries differ; first {bad[0]}: {a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}; "
                             f"max abs diff {np.abs(a.astype(np.float64) - b.astype(np.float64)).max():.3e} (tol {TOL})")


def test_geneaJi_reference_golden(gen):
    """test/runtests.jl:50-53 through the C-ABI: exact == on the pinned 3x3 and its mean."""
    ped = gen.genealogy(gen.geneaJi)
    phi = gen.phi(ped, verbose=True)
    _assert_equal(phi, np.array(GOLD["geneaJi"]["phi"], dtype=np.float32))
    assert float(gen.phiMean(phi)) == GOLD["geneaJi"]["phiMean"]


@pytest.mark.parametrize("kernel", [0, 1])
def test_genea140_bit_exact(gen, oracle, kernel):
    ped = gen.genealogy(gen.genea140)
    phi = gen.phi(ped, kernel=kernel)
    _assert_equal(phi, np.load(os.path.join(HERE, "golden", "genea140_phi_oracle.npy")))
    g = GOLD["genea140_survey_derived"]
    assert float(phi.astype(np.float64).sum()) == g["sum_all"]
    assert float(np.trace(phi.astype(np.float64))) == g["trace"]
    oped = oracle.Pedigree.from_file(gen.genea140)
    _assert_equal(phi, oped.phi())


def test_genea140_proband_subsets_and_shards(gen, oracle):
    ped = gen.genealogy(gen.genea140)
    oped = oracle.Pedigree.from_file(gen.genea140)
    pro = gen.pro(ped)
    rng = np.random.default_rng(3)
    sub = rng.permutation(pro)[:23]
    sub = np.concatenate([sub, sub[:2], [ped.father[np.flatnonzero(ped.ind == sub[3])[0]]]])  # dups + an ancestor
    _assert_equal(gen.phi(ped, sub), oped.phi(sub))
    # row shards (multi-GPU partition of the final level) reassemble to the full matrix
    pl = gen.plan(ped, pro)
    full = pl.compute()
    parts = [pl.compute(rows=(a, b)) for a, b in [(0, 50), (50, 51), (51, 140)]]
    _assert_equal(np.concatenate(parts, axis=0), full)
    pl.close()


@pytest.mark.parametrize("args,kw", [
    ((3000, 300, 12), dict(skip_permille=50)),
    ((5000, 500, 8), dict(skip_permille=0)),
    ((2000, 100, 25), dict(skip_permille=200, seed=7)),
    ((20000, 2000, 10), dict(skip_permille=0)),
])
def test_synthetic_random_mating_bit_exact(gen, oracle, args, kw):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(*args, **kw)
    for kernel in (0, 1):
        _assert_equal(_gpu_phi(gen, ind, fa, mo, sex, pro, kernel=kernel), oracle.Pedigree(ind, fa, mo).phi(pro))


def test_deep_inbred_float32_rounding_stress(gen, oracle):
    """cfg5 shape: 200 generations, most entries inexact on every Float32 store."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.deep_inbred(200, 50, 3)
    phi = _gpu_phi(gen, ind, fa, mo, sex, pro)
    _assert_equal(phi, oracle.Pedigree(ind, fa, mo).phi(pro))
    assert phi.diagonal().min() > 0.9


def test_fused_small_levels_match_per_level_launches(gen, oracle, monkeypatch):
    """Runs of level steps with cuts <= 128 members go through ONE persistent launch
    (levels_small_kernel, both matrices in LDS); bit-equal to per-level launches and the oracle."""
    from genlib_jl_amd import synth
    for args in ((200, 50, 3), (60, 120, 5), (40, 128, 7), (25, 130, 4)):      # 130: cuts straddle the limit
        ind, fa, mo, sex, pro = synth.deep_inbred(*args)
        ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
        want = oracle.Pedigree(ind, fa, mo).phi(pro)
        monkeypatch.delenv("GENPHI_NO_SMALL", raising=False)
        pl = gen.plan(ped, pro)
        fused = pl.compute(timing=True)
        ms = [pl.stats.level_ms[k] for k in range(pl.stats.n_steps)]
        sizes = pl.levels()[0]
        pl.close()
        _assert_equal(fused, want)
        if max(sizes[:-1]) <= 128:
            assert sum(1 for t in ms[:-1] if t == 0.0) >= len(ms) - 2, "the fused run books its time on one step"
        monkeypatch.setenv("GENPHI_NO_SMALL", "1")
        pl = gen.plan(ped, pro)
        _assert_equal(pl.compute(), want)
        pl.close()
    monkeypatch.delenv("GENPHI_NO_SMALL", raising=False)
    # the top levels of a real pedigree are small too (genea140 starts at 10 founders)
    ped = gen.genealogy(gen.genea140)
    _assert_equal(gen.phi(ped), np.load(os.path.join(HERE, "golden", "genea140_phi_oracle.npy")))


def test_first_level_from_indices_matches_materialised_identity(gen, oracle, monkeypatch):
    """Level step 0 reads Psi_1 = 1/2 I (src/compute.jl:271-274): level_identity_kernel computes
    it from the index arrays alone; the regular kernels on a materialised 1/2 I must agree."""
    from genlib_jl_amd import synth
    cases = [synth.random_mating(6000, 500, 4, skip_permille=100),      # step 0 in FULL mode, dragged rows
             synth.random_mating(40_000, 3000, 3),                      # wide first cut
             ]
    n = 700                                                             # founders only: no level step at all
    cases.append((np.arange(1, n + 1), np.zeros(n, np.int64), np.zeros(n, np.int64), np.ones(n, np.int64), np.arange(1, n + 1)))
    ind, fa, mo, sex, _ = synth.random_mating(3000, 300, 2)
    cases.append((ind, fa, mo, sex, ind[fa != 0][:200]))                # step 0 is also the last step
    for ind, fa, mo, sex, pro in cases:
        want = oracle.Pedigree(ind, fa, mo).phi(pro)
        for off in (False, True):
            if off:
                monkeypatch.setenv("GENPHI_NO_IDENTITY", "1")
            else:
                monkeypatch.delenv("GENPHI_NO_IDENTITY", raising=False)
            _assert_equal(_gpu_phi(gen, ind, fa, mo, sex, pro), want)
    monkeypatch.delenv("GENPHI_NO_IDENTITY", raising=False)
    ped = gen.genealogy(gen.geneaJi)
    pl = gen.plan(ped)
    full = pl.compute()
    pl.compute_device(rows=(1, 3))                                       # sharded last level, small
    assert np.array_equal(pl.result_to_host(), full[1:3])
    pl.close()


def test_subnormal_kinship_rare_branch(gen, oracle):
    """Kinships below 2^-126 must be stored as Float32 subnormals exactly like the reference
    (no flush-to-zero), and below 2^-149 round to zero the same way."""
    from genlib_jl_amd import synth
    for depth in (60, 68, 73, 80):
        ind, fa, mo, sex, pro = synth.chain_two_lines(depth)
        phi = _gpu_phi(gen, ind, fa, mo, sex, pro)
        _assert_equal(phi, oracle.Pedigree(ind, fa, mo).phi(pro))
    ind, fa, mo, sex, pro = synth.chain_two_lines(68)
    phi = _gpu_phi(gen, ind, fa, mo, sex, pro)
    assert 0 < phi[0, 1] < np.finfo(np.float32).tiny          # really is a subnormal


def test_edge_cases(gen, oracle):
    # all probands parentless -> 1/2 I
    tri = dict(ind=[1, 2, 3], father=[0, 0, 0], mother=[0, 0, 0], sex=[1, 2, 1])
    ped = gen.genealogy(tri)
    _assert_equal(gen.phi(ped, [3, 1]), 0.5 * np.eye(2, dtype=np.float32))
    # one-parent individuals, proband that is an ancestor of another, selfing, duplicates
    ind, fa, mo, sex = [1, 2, 3, 4, 5, 6, 7], [0, 0, 1, 3, 0, 4, 6], [0, 0, 2, 0, 4, 4, 5], [1, 2, 1, 1, 2, 1, 1]
    oped = oracle.Pedigree(ind, fa, mo)
    for pro in ([7], [5, 3, 5, 1], [7, 6, 4, 2], [1, 2], [6, 7, 3]):
        _assert_equal(_gpu_phi(gen, ind, fa, mo, sex, pro), oped.phi(pro))
    # empty proband list
    assert gen.phi(gen.genealogy(tri), []).shape == (0, 0)
    # IDs are Julia Int (64-bit) labels, not indices: sparse, huge and unordered IDs give the same matrix
    big = {0: 0, **{i: (i * 0x1F3D5B79 + 7) % (1 << 61) + (1 << 40) for i in ind}}
    ind2, fa2, mo2 = [big[i] for i in ind], [big[i] for i in fa], [big[i] for i in mo]
    for pro in ([7, 6, 4, 2], [6, 7, 3]):
        _assert_equal(_gpu_phi(gen, ind2, fa2, mo2, sex, [big[i] for i in pro]), oped.phi(pro))


def test_wide_mode_forced_small_windows(gen, oracle, monkeypatch):
    """SPLIT (one source row in LDS at a time) and WIDE (block assembly from streaming passes, proband-order
    delivery pass) levels, forced on small inputs by shrinking the LDS budget; several chunks per row."""
    from genlib_jl_amd import synth
    modes_seen = set()
    for cap, args, kw in [(2048, (6000, 700, 7), dict(skip_permille=30)),
                          (1200, (6000, 700, 7), dict(skip_permille=30)),
                          (512, (6000, 700, 7), dict(skip_permille=0)),
                          (256, (3000, 300, 12), dict(skip_permille=100, seed=11))]:
        monkeypatch.setenv("GENPHI_LDS_CAP_FLOATS", str(cap))
        ind, fa, mo, sex, pro = synth.random_mating(*args, **kw)
        ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
        pl = gen.plan(ped, pro)
        modes_seen |= set(pl.step_modes())
        _assert_equal(pl.compute(), oracle.Pedigree(ind, fa, mo).phi(pro))
        pl.close()
    assert modes_seen == {0, 1, 2}          # FULL, SPLIT and HALF kernels all exercised
    monkeypatch.setenv("GENPHI_LDS_CAP_FLOATS", "1024")
    ped = gen.genealogy(gen.genea140)
    _assert_equal(gen.phi(ped), np.load(os.path.join(HERE, "golden", "genea140_phi_oracle.npy")))
    pl = gen.plan(ped)
    parts = [pl.compute(rows=(a, b)) for a, b in [(0, 33), (33, 140)]]
    _assert_equal(np.concatenate(parts, axis=0), np.load(os.path.join(HERE, "golden", "genea140_phi_oracle.npy")))
    pl.close()


def test_row_shards_compute_only_their_ancestors(gen, oracle, monkeypatch):
    """Multi-GPU partition: a rank computes, at every upper level, only the rows its shard of
    the last level descends from.  Shards must still reassemble to the full matrix bit for bit,
    in every kernel mode, and agree with the unpruned sweep."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(8000, 900, 9, skip_permille=40)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    want = oracle.Pedigree(ind, fa, mo).phi(pro)
    n = len(pro)
    cuts = [(0, 1), (1, 130), (130, 131), (131, 600), (600, n)]
    for cap in (None, 2048, 300):                         # FULL / SPLIT / HALF on the same pedigree
        if cap is None:
            monkeypatch.delenv("GENPHI_LDS_CAP_FLOATS", raising=False)
        else:
            monkeypatch.setenv("GENPHI_LDS_CAP_FLOATS", str(cap))
        for prune in (True, False):
            if prune:
                monkeypatch.delenv("GENPHI_NO_SHARD_PRUNE", raising=False)
            else:
                monkeypatch.setenv("GENPHI_NO_SHARD_PRUNE", "1")
            pl = gen.plan(ped, pro)
            parts = [pl.compute(rows=r) for r in cuts]
            _assert_equal(np.concatenate(parts, axis=0), want)
            _assert_equal(pl.compute(), want)             # back to the full sweep on the same plan
            _assert_equal(pl.compute(rows=(5, 17)), want[5:17])
            pl.close()
    monkeypatch.delenv("GENPHI_LDS_CAP_FLOATS", raising=False)
    monkeypatch.delenv("GENPHI_NO_SHARD_PRUNE", raising=False)
    # a shard whose ancestry stops early: above that, its levels have NO rows to compute, but the
    # level below still reads their all-zero "none" row for its parentless members (found by
    # tests/stress_random.py: stale rows of the previous sweep were read instead)
    deep = synth.deep_inbred(60, 30, 3)                                  # 60 generations, shared ancestry
    shallow = synth.deep_inbred(12, 24, 2, seed=5)                       # an unrelated family, 12 generations
    n1 = len(deep[0])
    rel = lambda a: np.where(a > 0, a + n1, 0)                           # noqa: E731  (relabel its IDs)
    ind = np.concatenate([deep[0], shallow[0] + n1])
    fa = np.concatenate([deep[1], rel(shallow[1])])
    mo = np.concatenate([deep[2], rel(shallow[2])])
    sex = np.concatenate([deep[3], shallow[3]])
    pro = np.concatenate([deep[4], shallow[4] + n1])
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    want = oracle.Pedigree(ind, fa, mo).phi(pro)
    for small_off in (False, True):
        if small_off:
            monkeypatch.setenv("GENPHI_NO_SMALL", "1")
        pl = gen.plan(ped, pro)
        _assert_equal(pl.compute(), want)                                # leaves every buffer full of old rows
        k = len(deep[4])
        _assert_equal(pl.compute(rows=(k, len(pro))), want[k:])          # only the shallow family
        _assert_equal(pl.compute(rows=(0, k)), want[:k])
        _assert_equal(pl.compute(rows=(k - 3, k + 5)), want[k - 3:k + 5])
        pl.close()
    monkeypatch.delenv("GENPHI_NO_SMALL", raising=False)
    # a shard really does less work above the last level: compare level times at cfg3 size
    ind, fa, mo, sex, pro = synth.random_mating(100_000, 10_000, 20)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    pl.compute_device(timing=True)
    full_ms = sum(pl.stats.level_ms[k] for k in range(10, pl.stats.n_steps - 1))
    for _ in range(2):
        pl.compute_device(rows=(0, 1250), timing=True)
    shard_ms = sum(pl.stats.level_ms[k] for k in range(10, pl.stats.n_steps - 1))
    pl.close()
    assert shard_ms < 0.97 * full_ms, (shard_ms, full_ms)


def test_cfg3_full_size_bit_exact(gen, oracle, monkeypatch):
    """cfg3 at full size (1e5 individuals / 1e4 probands / 20 generations) against the oracle (C/OpenMP: a
    few seconds), bit for bit: the default kernels (FULL levels), the same pedigree with every level forced
    through the SPLIT kernels (certified-rows kernel, then the grouping-exact one), the naive kernel, and
    the size-independent properties (symmetry, diagonal range)."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(100_000, 10_000, 20)
    want = oracle.Pedigree(ind, fa, mo).phi(pro)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    assert set(pl.step_modes()) == {0}
    a = pl.compute(kernel=0)
    b = pl.compute(kernel=1)
    pl.close()
    _assert_equal(a, want)
    _assert_equal(b, want)
    assert np.array_equal(a, a.T)
    d = a.diagonal()
    assert d.min() >= 0.5 and d.max() < 1.0
    assert a.min() >= 0.0 and (a - np.diag(d)).max() <= 0.5
    monkeypatch.setenv("GENPHI_FULL_MAX_FLOATS", "0")
    for env in ({}, {"GENPHI_NO_FAST": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        pl = gen.plan(ped, pro)
        assert set(pl.step_modes()) == {1}
        _assert_equal(pl.compute(), want)
        pl.close()
    for k in ("GENPHI_FULL_MAX_FLOATS", "GENPHI_NO_FAST"):
        monkeypatch.delenv(k, raising=False)


def test_cfg4_shaped_mid_size_bit_exact(gen, oracle):
    """The headline configuration's kernel geometry at a size the oracle still does in about a minute: 1.6e5
    individuals / 2.9e4 probands / 6 generations -- cuts of ~20k members (SPLIT by default: the 1024-thread
    certified-rows kernel, 80 KB source rows) and a final level of 2.9e4 columns (512-thread kernel, two column
    chunks per row), default settings, no test hooks.  Full matrix and two row shards, bit for bit."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(160_000, 29_000, 6)
    want = oracle.Pedigree(ind, fa, mo).phi(pro)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    assert set(pl.step_modes()) == {1} and len(want) == 29_000
    _assert_equal(pl.compute(), want)
    parts = [pl.compute(rows=r) for r in [(0, 9_000), (9_000, 29_000)]]
    _assert_equal(np.concatenate(parts, axis=0), want)
    pl.close()


def test_wide_cuts_at_real_size_default_settings(gen, oracle):
    """WIDE levels without any test hook: overlapping generations (40 % of the parents from g-2) make cuts of
    39.6k, 48.0k and 37.0k members, wider than the 36 864 floats of LDS a source row may take.  The plan holds a
    WIDE step whose new x new block is a SPLIT sub-step written in place, one whose parents are too many for
    that (per-entry kernel on the block), and a WIDE last step (proband-order delivery); bit for bit against
    the oracle (about a minute of CPU), plus a row shard."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(150_000, 30_000, 5, skip_permille=400)
    want = oracle.Pedigree(ind, fa, mo).phi(pro)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    modes = pl.step_modes()
    assert modes == [1, 2, 2, 2] and max(pl.levels()[0]) > 36_864
    assert {pl.step_info(k)[3] for k in range(1, 4)} == {1, 3}           # SPLIT sub-step and per-entry fallback
    _assert_equal(pl.compute(), want)
    _assert_equal(pl.compute(rows=(5_000, 5_700)), want[5_000:5_700])
    pl.close()


def test_wide_in_place_at_real_size_default_settings(gen, oracle):
    """In-place levels at WIDE width against the ORACLE with no test hook: 1.5e5 individuals / 8,000 probands / 12 generations,
    20 % of the parents from g-2 -- cuts to 42,298 members (a source row does not fit in LDS), five steps in place, their source cuts
    28.6k to 42.3k members wide (three of them wider than the 36,864 floats of LDS), the rest of the plan at SPLIT width; bit for bit (4.1e9 pair evaluations on the host, ~40 s), plus
    a row shard and the per-entry kernel sweep on the same plan."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(150_000, 8_000, 12, skip_permille=200)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    sizes, both = pl.levels()
    flags = [pl.step_slots(k) for k in range(len(sizes) - 1)]
    stay = [k for k, f in enumerate(flags) if f[0] & 1]
    assert max(sizes) > 36_864 and len(stay) >= 5 and sum(sizes[k] > 36_863 for k in stay) >= 2, (sizes, flags)
    want = oracle.Pedigree(ind, fa, mo).phi(pro)
    for rep in range(3):
        _assert_equal(pl.compute(), want)
    _assert_equal(pl.compute(rows=(1_000, 1_900)), want[1_000:1_900])
    _assert_equal(pl.compute(kernel=1), want)
    pl.close()


def test_real_genealogy_every_individual_a_proband(gen, oracle, monkeypatch):
    """The full kinship matrix of a genealogy: genea140 with EVERY one of its 41,523 individuals a proband (nobody ever leaves the
    cuts: B = 101 GB, nearly all of it dragged x dragged copy, src/compute.jl:108-110).  Default settings: eleven steps in place,
    the proband cut included -- its step writes the last 140 rows and columns and the result is DELIVERED from the slot matrix by one
    permutation pass (Plan::final_slots).  Bit for bit against the oracle (6.7e9 pair evaluations, ~50 s), the whole 41,523 x 41,523
    matrix; a row shard; and a random quarter of the individuals (10,380 probands, ancestors among them at every depth) with the
    proband cut in place or not (GENPHI_STAY_LAST=0) and with nothing in place."""
    ped = gen.genealogy(gen.genea140)
    oped = oracle.Pedigree.from_file(gen.genea140)
    ids = np.asarray(ped.ind, dtype=np.int64)
    pl = gen.plan(ped, ids)
    sizes, both = pl.levels()
    flags = [pl.step_slots(k) for k in range(len(sizes) - 1)]
    assert pl.n_probands == 41_523 and sum(f[0] & 1 for f in flags) >= 10 and flags[-1][0] & 1      # the last step stays in place too
    want = oped.phi(ids)
    got = pl.compute()
    assert got.shape == want.shape and np.array_equal(got, want)
    _assert_equal(pl.compute(rows=(20_000, 20_300)), want[20_000:20_300])
    _assert_equal(pl.compute(rows=(41_000, 41_523)), want[41_000:])
    pl.close()
    del got
    sub = np.sort(np.random.default_rng(7).choice(ids, size=len(ids) // 4, replace=False))
    wsub = oped.phi(sub)
    for env in ({}, {"GENPHI_STAY_LAST": "0"}, {"GENPHI_STAY_NARROW": "2"}, {"GENPHI_STAY_NARROW": "2", "GENPHI_CERT_MIN_EXP": "-6"}, {"GENPHI_NO_STAY": "1"}):
        for k in ("GENPHI_STAY_LAST", "GENPHI_STAY_NARROW", "GENPHI_NO_STAY", "GENPHI_CERT_MIN_EXP"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        pl = gen.plan(ped, sub)
        for rep in range(3):
            _assert_equal(pl.compute(), wsub)
        _assert_equal(pl.compute(kernel=1), wsub)
        _assert_equal(pl.compute(rows=(5_000, 5_700)), wsub[5_000:5_700])
        pl.close()
    for k in ("GENPHI_STAY_LAST", "GENPHI_STAY_NARROW", "GENPHI_NO_STAY", "GENPHI_CERT_MIN_EXP"):
        monkeypatch.delenv(k, raising=False)


def test_many_probands_from_few_parents(gen, oracle, monkeypatch):
    """A final level much wider than the cut above it (1100 parents, 20 000 probands: 18 children per
    parent): the FULL kernel walks 20 000 columns per row from two 4.4 KB source rows; the same pedigree
    through the SPLIT kernels (5 column chunks at the forced 4 columns per thread); row shards."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(22_200, 20_000, 3)
    want = oracle.Pedigree(ind, fa, mo).phi(pro)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    assert pl.step_modes() == [0, 0] and pl.levels()[0][-2] < 1200
    _assert_equal(pl.compute(), want)
    _assert_equal(pl.compute(rows=(123, 4567)), want[123:4567])
    pl.close()
    monkeypatch.setenv("GENPHI_FULL_MAX_FLOATS", "0")
    monkeypatch.setenv("GENPHI_NO_SMALL", "1")
    monkeypatch.setenv("GENPHI_MAX_CPT", "4")
    pl = gen.plan(ped, pro)
    assert pl.step_modes() == [1, 1]
    _assert_equal(pl.compute(), want)
    pl.close()
    for k in ("GENPHI_FULL_MAX_FLOATS", "GENPHI_NO_SMALL", "GENPHI_MAX_CPT"):
        monkeypatch.delenv(k, raising=False)


def test_huge_sibships_through_the_split_kernels(gen, oracle, monkeypatch):
    """Three sires per generation of 600 (sibships of ~200 by one father: sibling groups are cut every 8
    rows, consecutive groups share their A row), heavy inbreeding (most stores inexact), every level forced
    through the SPLIT kernels: certified-rows kernel where the rows qualify, grouping-exact kernel for the
    rest and, hook, for everything."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.deep_inbred(25, 600, 3)
    want = oracle.Pedigree(ind, fa, mo).phi(pro)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    monkeypatch.setenv("GENPHI_FULL_MAX_FLOATS", "0")
    monkeypatch.setenv("GENPHI_NO_SMALL", "1")
    for env in ({}, {"GENPHI_NO_FAST": "1"}, {"GENPHI_MAX_GROUP": "3"}, {"GENPHI_FAST_NT": "512", "GENPHI_CERT_MIN_EXP": "-2"}):
        for k in ("GENPHI_NO_FAST", "GENPHI_MAX_GROUP", "GENPHI_FAST_NT", "GENPHI_CERT_MIN_EXP"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        pl = gen.plan(ped, pro)
        assert set(pl.step_modes()) == {1}
        _assert_equal(pl.compute(), want)
        _assert_equal(pl.compute(rows=(7, 311)), want[7:311])
        pl.close()
    for k in ("GENPHI_NO_FAST", "GENPHI_MAX_GROUP", "GENPHI_FAST_NT", "GENPHI_CERT_MIN_EXP", "GENPHI_FULL_MAX_FLOATS", "GENPHI_NO_SMALL"):
        monkeypatch.delenv(k, raising=False)


def test_result_to_host_symmetric_copy(gen, oracle, monkeypatch):
    """genphi_result_to_host of a FULL result moves only the tiles on and above the diagonal across the link and mirrors them on
    the host (the matrix is bit-symmetric; the reference returns the full Matrix{Float32}, src/compute.jl:303): forced here on
    small results with odd tile shapes (several column tiles per row block, ragged last tiles, tiles wider than the matrix, a
    single thread), == the plain copy (GENPHI_D2H_SYM=0) == the oracle; row shards keep the plain copy."""
    from genlib_jl_amd import synth
    for args, kw in [((9000, 2501, 6), dict(skip_permille=30)), ((3000, 97, 5), dict()), ((400, 3, 4), dict())]:
        ind, fa, mo, sex, pro = synth.random_mating(*args, **kw)
        ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
        want = oracle.Pedigree(ind, fa, mo).phi(pro)
        assert np.array_equal(want, want.T)
        for env in ({"GENPHI_D2H_SYM": "0"}, {"GENPHI_D2H_SYM": "1"}, {"GENPHI_D2H_SYM": "1", "GENPHI_D2H_TILE": "96x700", "GENPHI_D2H_THREADS": "5"},
                    {"GENPHI_D2H_SYM": "1", "GENPHI_D2H_TILE": "33x64", "GENPHI_D2H_THREADS": "1"},
                    {"GENPHI_D2H_SYM": "1", "GENPHI_D2H_TILE": "1000x50", "GENPHI_D2H_THREADS": "3"}):
            for k in ("GENPHI_D2H_SYM", "GENPHI_D2H_TILE", "GENPHI_D2H_THREADS"):
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            pl = gen.plan(ped, pro)
            for rep in range(2):
                got = np.full_like(want, np.float32(-7.0))
                pl.compute_device()
                got[...] = pl.result_to_host()
                _assert_equal(got, want)
            n = len(want)
            _assert_equal(pl.compute(rows=(n // 3, n)), want[n // 3:])          # a shard is not symmetric by itself: plain copy
            _assert_equal(pl.compute(), want)
            pl.close()
    for k in ("GENPHI_D2H_SYM", "GENPHI_D2H_TILE", "GENPHI_D2H_THREADS"):
        monkeypatch.delenv(k, raising=False)


def test_phi_mean_on_device(gen, oracle):
    """phiMean reduced on the device (no 40 GB device-to-host copy)."""
    ped = gen.genealogy(gen.geneaJi)
    pl = gen.plan(ped)
    phi = pl.compute()
    assert float(pl.phi_mean()) == GOLD["geneaJi"]["phiMean"]            # test/runtests.jl:53, exact
    a, d, nr = pl.result_sums()
    assert a == float(phi.astype(np.float64).sum()) and d == float(np.trace(phi.astype(np.float64))) and nr == 3
    pl.close()
    ped = gen.genealogy(gen.genea140)
    pl = gen.plan(ped)
    phi = pl.compute()
    g = GOLD["genea140_survey_derived"]
    a, d, _ = pl.result_sums()
    assert abs(a - g["sum_all"]) <= 1e-12 * g["sum_all"] and abs(d - g["trace"]) <= 1e-12 * g["trace"]
    assert abs(float(pl.phi_mean()) - float(gen.phiMean(phi))) <= 1e-9   # host Float32 mirror vs device Float64
    # shards: partial sums add up
    parts = []
    for r in [(0, 60), (60, 140)]:
        pl.compute_device(rows=r)
        parts.append(pl.result_sums())
    assert abs(sum(p[0] for p in parts) - a) <= 1e-12 * a and abs(sum(p[1] for p in parts) - d) <= 1e-12 * d
    pl.close()


def test_inbreeding_f_from_the_sweep(gen, oracle):
    """gen.f(pedigree, IDs) (src/compute.jl:500-511) from ONE Float64 level sweep
    over the parents + point lookups (genphi_result_entries) instead of the exponential pairwise
    recursion -- bit-equal to the recursion (oracle.f restates :66-95 and :500-511 literally)."""
    ped = gen.genealogy(gen.geneaJi)
    assert gen.f(ped, [1]).tolist() == [GOLD["geneaJi"]["f_1"]]            # test/runtests.jl:47, exact
    assert gen.f(ped, [17]).tolist() == [GOLD["geneaJi"]["f_17"]]          # :48
    assert gen.f(ped, [1]).dtype == np.float32
    op = oracle.Pedigree.from_file(gen.geneaJi)
    assert np.array_equal(gen.f(ped, ped.ind), op.f(ped.ind))              # every individual
    with pytest.raises(KeyError):
        gen.f(ped, [424242])
    # genea140, all 140 probands: bit-equal to the exact Float64 recursion rounded once (north-star
    # tolerance 1e-12: the difference is exactly 0), where the Float32-per-level sweep is off by up to 3e-8
    ped = gen.genealogy(gen.genea140)
    op = oracle.Pedigree.from_file(gen.genea140)
    ids = gen.pro(ped)
    got = gen.f(ped, ids)
    want = op.f(ids)
    assert got.dtype == want.dtype == np.float32
    assert np.array_equal(got, want), np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    assert np.count_nonzero(got) > 100
    pos = ped.positions(ids)
    fa, mo = ped.father[pos], ped.mother[pos]
    parents = np.unique(np.concatenate([fa, mo]))
    sweep32 = gen.phi(ped, parents)[np.searchsorted(parents, fa), np.searchsorted(parents, mo)]
    assert np.abs(sweep32.astype(np.float64) - want.astype(np.float64)).max() <= 4e-8          # what round 1 returned
    # a random pedigree with one-parent individuals and overlapping generations
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(3000, 300, 9, skip_permille=120, seed=4)
    mo = mo.copy(); mo[::17] = 0                                           # one-parent rows (father only)
    ped2 = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    op2 = oracle.Pedigree(ind, fa, mo)
    some = np.concatenate([pro[:60], ind[1500:1530]])
    assert np.array_equal(gen.f(ped2, some), op2.f(some))
    # point lookups: any entry of a resident (sharded) result
    pl = gen.plan(ped)
    full = pl.compute()
    r = np.array([0, 5, 139, 77]); c = np.array([139, 5, 0, 12])
    assert np.array_equal(pl.result_entries(r, c), full[r, c].astype(np.float64))
    pl.compute_device(rows=(60, 140))
    assert np.array_equal(pl.result_entries([60, 139], [3, 139]), full[[60, 139], [3, 139]].astype(np.float64))
    with pytest.raises(ValueError):
        pl.result_entries([10], [3])                                       # row not resident
    pl.close()


def test_random_pedigrees_bit_exact(gen, oracle, monkeypatch):
    """Randomised structures the synthetic shapes never produce, through every kernel mode."""
    rng = np.random.default_rng(20241016)
    cases = 0
    for cap in (None, 640, 200):
        if cap is None:
            monkeypatch.delenv("GENPHI_LDS_CAP_FLOATS", raising=False)
        else:
            monkeypatch.setenv("GENPHI_LDS_CAP_FLOATS", str(cap))
        for n, pf, p1, ps, back in [(60, 0.2, 0.2, 0.1, 8), (400, 0.05, 0.1, 0.02, 40), (1500, 0.02, 0.05, 0.0, 300),
                                    (1500, 0.3, 0.3, 0.05, 1500), (800, 0.01, 0.0, 0.0, 60)]:
            ind, fa, mo, sex = _random_pedigree(rng, n, pf, p1, ps, back)
            oped = oracle.Pedigree(ind, fa, mo)
            ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
            assert np.array_equal(ped.ind, oped.ind)
            for pro in (None, rng.choice(ind, size=min(n, 37), replace=True)):
                pro = oped.pro() if pro is None else pro
                pl = gen.plan(ped, pro)
                sizes, both = pl.levels()
                osz, obo, _ = oped.levels(pro)
                assert sizes == osz and both == obo
                _assert_equal(pl.compute(), oped.phi(pro))
                pl.close()
                cases += 1
    assert cases == 30


def test_random_stress_short(gen):
    """A short fixed-seed run of tests/stress_random.py (random pedigree x kernel mode x proband
    subset x three random row shards x replay / naive kernel / lookups / sums, all against the
    oracle); the long runs of that script are what found the empty-level bug of the shard pruning."""
    import subprocess, sys
    out = subprocess.run([sys.executable, os.path.join(HERE, "stress_random.py"), "25", "2024"], cwd=HERE,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert ", 0 failures" in out.stdout.splitlines()[-1], out.stdout[-2000:]


def test_graph_replay_matches_eager(gen, oracle):
    """The sweep is replayed from a captured hipGraph from the second untimed compute on:
    results must not change, also after switching shard / kernel and back."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.deep_inbred(120, 40, 3)
    ref = oracle.Pedigree(ind, fa, mo).phi(pro)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    for _ in range(4):                                   # eager, capture + replay, replay, replay
        _assert_equal(pl.compute(), ref)
    _assert_equal(pl.compute(rows=(5, 17)), ref[5:17])   # new key: eager again
    _assert_equal(pl.compute(rows=(5, 17)), ref[5:17])   # captured for the shard
    _assert_equal(pl.compute(kernel=1), ref)
    _assert_equal(pl.compute(), ref)
    _assert_equal(pl.compute(), ref)
    st = pl.compute_device(timing=True)                  # timing runs stay eager
    assert st.timed == 1 and st.n_steps == len(pl.levels()[0]) - 1
    _assert_equal(pl.result_to_host(), ref)
    pl.close()


def test_step_hook_is_called_before_every_level_step(gen, oracle, capsys):
    """genphi_plan_set_step_hook: the reference prints "Running step k of n (...)" INSIDE its level loop (src/compute.jl:280-285);
    the library calls the hook right before it hands each level step to the GPU -- every step once, in order, also for the steps a
    fused small-level run covers and on repeated sweeps (a hooked sweep is never replayed from a graph); results unchanged."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.deep_inbred(40, 30, 3)
    ref = oracle.Pedigree(ind, fa, mo).phi(pro)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    n_steps = len(pl.levels()[0]) - 1
    seen = []
    pl.set_step_hook(lambda k, n: seen.append((k, n)))
    for rep in range(3):
        _assert_equal(pl.compute(), ref)
    assert seen == [(k, n_steps) for k in range(n_steps)] * 3
    pl.set_step_hook(None)
    _assert_equal(pl.compute(), ref)
    assert len(seen) == 3 * n_steps
    pl.close()
    # the Python mirror prints the reference's lines through it
    ped = gen.genealogy(gen.geneaJi)
    gen.phi(ped, verbose=True)
    out = capsys.readouterr().out.splitlines()
    assert out[:7] == [f"Step {i} of 7: {a} founders, {b} probands, {c} both." for i, (a, b, c) in
                       enumerate([(2, 4, 2), (4, 6, 4), (6, 7, 4), (7, 9, 4), (9, 8, 0), (8, 4, 0), (4, 3, 0)], 1)]
    assert out[7:] == [f"Running step {i} of 7 ({a} founders, {b} probands, {c} both)." for i, (a, b, c) in
                       enumerate([(2, 4, 2), (4, 6, 4), (6, 7, 4), (7, 9, 4), (9, 8, 0), (8, 4, 0), (4, 3, 0)], 1)]


def test_full_size_cfg4_properties(gen):
    """BASELINE.json's headline size (1e6 individuals / 1e5 probands / 30 generations): far too
    big for the oracle, so check size-independent properties of the 40 GB result without moving
    it to the host: (i) the Float64 row-sum checksums of the pipelined kernel and of the naive
    one-thread-per-entry kernel are bit-identical; (ii) shard checksums add up to the full one;
    (iii) symmetry and diagonal range on sampled row blocks fetched through the shard API."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(1_000_000, 100_000, 30)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    n = pl.n_probands
    assert n == 100_000 and set(pl.step_modes()) == {1}           # every level through the SPLIT kernel
    pl.compute_device()
    full = pl.result_sums()
    mean = float(pl.phi_mean())
    assert 0.0 < mean < 0.01
    pl.compute_device(kernel=1)
    assert pl.result_sums() == full                                # naive kernel: identical checksums
    parts = []
    for r in [(0, 30_000), (30_000, 30_001), (30_001, 100_000)]:
        pl.compute_device(rows=r)
        parts.append(pl.result_sums())
    assert sum(p[2] for p in parts) == n
    assert abs(sum(p[0] for p in parts) - full[0]) <= 1e-12 * full[0]
    assert sum(p[1] for p in parts) == full[1]                     # diagonals are dyadic: exact in any order
    a = pl.compute(rows=(1000, 1064))                              # (64, n)
    b = pl.compute(rows=(77_000, 77_064))
    assert np.array_equal(a[:, 77_000:77_064], b[:, 1000:1064].T)  # bit-symmetric
    d = np.concatenate([a[np.arange(64), 1000 + np.arange(64)], b[np.arange(64), 77_000 + np.arange(64)]])
    assert d.min() >= 0.5 and d.max() < 1.0 and a.min() >= 0.0 and a.max() < 1.0
    pl.close()


def _resident_rows(pl, rows, chunk=32):
    """Rows `rows` of the resident N x N result (after a full compute_device) without copying the matrix: point lookups."""
    n = pl.n_probands
    out = np.empty((len(rows), n), dtype=np.float32)
    cols = np.arange(n, dtype=np.int64)
    for a in range(0, len(rows), chunk):
        rr = np.asarray(rows[a:a + chunk], dtype=np.int64)
        got = pl.result_entries(np.repeat(rr, n), np.tile(cols, len(rr)))
        out[a:a + len(rr)] = got.reshape(len(rr), n).astype(np.float32)          # (Float32 values read as Float64: exact)
    return out


def test_full_size_cfg4_oracle_row_sample(gen):
    """The headline configuration at FULL size (1e6 individuals / 1e5 probands / 30 generations, the bench's default workload)
    against the ORACLE, not against another HIP kernel: tests/golden/cfg4_rowsample.npz holds 158 rows of the 1e5 x 1e5 proband
    matrix as the oracle computes them -- every upper level step of src/compute.jl:291-299 restated in full on the host (8.3e9 pair
    evaluations; tests/golden/make_rowsamples.py, 170 s on 8 cores) -- as SHA-256 per row, Float64 sums per row and per block of 4,096
    columns.  The first and the last rows of the last step's work queue, rows spread over the proband order, three consecutive rows;
    compared bit for bit (the hash) with the same rows of the matrix the default sweep left in HBM: sparse leading cuts, the dense
    upper levels, the 4-chunk <512, 52, 16> instantiation of the certified-rows kernel in the last level (every row crosses all
    four column chunks).  The same with every level dense (GENPHI_FLAG_NO_SPARSE) and as a row shard."""
    import hashlib
    from genlib_jl_amd import synth
    fx = np.load(os.path.join(HERE, "golden", "cfg4_rowsample.npz"))
    rows, block = fx["rows"].astype(np.int64), int(fx["block"])
    ind, fa, mo, sex, pro = synth.random_mating(1_000_000, 100_000, 30)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    n = pl.n_probands
    modes = pl.step_modes()
    assert n == 100_000 and set(modes) == {1}
    desc, seg, run = pl.step_walk(len(modes) - 1)
    order = desc[:, 1].astype(np.int64)                              # output rows in work-queue order
    assert set(order[:48]) <= set(rows) and set(order[-48:]) <= set(rows), "the fixture samples the ends of THIS plan's work queue"

    def check(got, which):
        for k, r in enumerate(which):
            if hashlib.sha256(np.ascontiguousarray(got[k]).tobytes()).hexdigest() != str(fx["sha256"][r]):
                bs = np.array([got[k, b * block:(b + 1) * block].astype(np.float64).sum() for b in range(fx["block_sum"].shape[1])])
                bad = np.flatnonzero(bs != fx["block_sum"][r])
                raise AssertionError(f"row {rows[r]} differs from the oracle's: column blocks {bad.tolist()} (of {block}); row sum {got[k].astype(np.float64).sum()!r} "
                                     f"vs {float(fx['row_sum'][r])!r}; first entries {got[k, :4]} vs {fx['head'][r, :4]} (tol {TOL})")

    for no_sparse in (False, True):
        pl.compute_device(no_sparse=no_sparse)
        if not no_sparse:
            assert pl.sparse_levels()[0] >= 4, pl.sparse_levels()
        check(_resident_rows(pl, rows), range(len(rows)))
    # the same rows as a row shard of their own (shard work lists, pruned upper levels)
    k0 = int(np.searchsorted(rows, 50_000))
    assert list(rows[k0:k0 + 3]) == [50_000, 50_001, 50_002]
    check(pl.compute(rows=(50_000, 50_003)), range(k0, k0 + 3))
    pl.close()


def test_full_size_cfg4o_properties(gen):
    """The overlapping-generations workload of the bench at full size (1e6 individuals / 1e5 probands, 0.5 % of the
    parents from g-2: cuts to 123.5k members, 23 WIDE levels, both routes for the dragged blocks, source
    positions beyond 16 bits): the Float64 row-sum checksums of the block-assembly kernels and of the
    one-thread-per-entry kernel are bit-identical, and sampled row blocks are bit-symmetric."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(1_000_000, 100_000, 30, skip_permille=5)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    n = pl.n_probands
    modes = pl.step_modes()
    assert n == 100_000 and modes.count(2) == 23 and max(pl.levels()[0]) > 120_000
    pl.compute_device()
    full = pl.result_sums()
    pl.compute_device(kernel=1)
    assert pl.result_sums() == full                                # per-entry kernel: identical checksums
    a = pl.compute(rows=(2000, 2064))
    b = pl.compute(rows=(91_000, 91_064))
    assert np.array_equal(a[:, 91_000:91_064], b[:, 2000:2064].T)  # bit-symmetric
    d = np.concatenate([a[np.arange(64), 2000 + np.arange(64)], b[np.arange(64), 91_000 + np.arange(64)]])
    assert d.min() >= 0.5 and d.max() < 1.0 and a.min() >= 0.0 and a.max() < 1.0
    pl.close()


def _merge(peds):
    """Disjoint union of (ind, father, mother, sex, pro) pedigrees, IDs relabelled."""
    ind, fa, mo, sex, pro, off = [], [], [], [], [], 0
    for i, f, m, s, p in peds:
        i, f, m, s, p = (np.asarray(x, dtype=np.int64) for x in (i, f, m, s, p))
        rel = lambda a: np.where(a > 0, a + off, 0)                        # noqa: E731
        ind.append(i + off); fa.append(rel(f)); mo.append(rel(m)); sex.append(s); pro.append(p + off)
        off += int(i.max())
    return tuple(np.concatenate(x) for x in (ind, fa, mo, sex, pro))


def test_certified_rows_fast_path_and_mixed_levels(gen, oracle, monkeypatch):
    """SPLIT levels run two kernels: sibling groups whose source rows all carry the exactness
    certificate (entries 0 or >= 2^-27: every Float64 partial sum exact, so the reference's grouping
    cannot matter) take level_split_fast_kernel, the others the grouping-exact level_split_kernel;
    the split is made on the device per launch.  All of: certified only, uncertified only, mixed
    (threshold raised by the test hook; really tiny kinships), 512- and 1024-thread variants, row
    shards -- must equal the oracle bit for bit."""
    from genlib_jl_amd import synth
    base = synth.random_mating(6000, 700, 7, skip_permille=30)
    tiny = synth.chain_two_lines(22)                                       # kinship 2^-45: no certificate
    tiny2 = synth.chain_two_lines(40)
    cases = [base, _merge([base, tiny, tiny2]), synth.random_mating(3000, 300, 12, skip_permille=100, seed=11)]
    monkeypatch.setenv("GENPHI_FULL_MAX_FLOATS", "0")                      # no FULL kernel: every level is SPLIT
    monkeypatch.setenv("GENPHI_NO_SMALL", "1")
    for ind, fa, mo, sex, pro in cases:
        want = oracle.Pedigree(ind, fa, mo).phi(pro)
        ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
        for cap in (8192, 1024):                                          # one / several column chunks
            monkeypatch.setenv("GENPHI_LDS_CAP_FLOATS", str(cap))
            for env in ({}, {"GENPHI_NO_FAST": "1"}, {"GENPHI_CERT_MIN_EXP": "-9"}, {"GENPHI_CERT_MIN_EXP": "-4"},
                        {"GENPHI_CERT_MIN_EXP": "-1"}, {"GENPHI_FAST_NT": "512"}, {"GENPHI_FAST_NT": "512", "GENPHI_CERT_MIN_EXP": "-5"},
                        {"GENPHI_MAX_CPT": "8", "GENPHI_CERT_MIN_EXP": "-6"}, {"GENPHI_FAST_NT": "512", "GENPHI_MAX_CPT": "4"},
                        # the hub walk chaining from hub to hub (runs of several segments, chain steps), certified and mixed
                        {"GENPHI_MAX_RUN": "32"}, {"GENPHI_MAX_RUN": "6", "GENPHI_CERT_MIN_EXP": "-5"},
                        {"GENPHI_MAX_RUN": "100", "GENPHI_FAST_NT": "512", "GENPHI_MAX_GROUP": "2"}):
                for k in ("GENPHI_NO_FAST", "GENPHI_CERT_MIN_EXP", "GENPHI_FAST_NT", "GENPHI_MAX_CPT", "GENPHI_MAX_RUN", "GENPHI_MAX_GROUP"):
                    monkeypatch.delenv(k, raising=False)
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                pl = gen.plan(ped, pro)
                assert 1 in pl.step_modes() and 0 not in pl.step_modes()
                _assert_equal(pl.compute(), want)
                n = len(want)
                parts = [pl.compute(rows=r) for r in [(0, n // 3), (n // 3, n // 3 + 1), (n // 3 + 1, n)]]
                _assert_equal(np.concatenate(parts, axis=0), want)
                pl.close()
    for k in ("GENPHI_NO_FAST", "GENPHI_CERT_MIN_EXP", "GENPHI_FAST_NT", "GENPHI_MAX_CPT", "GENPHI_FULL_MAX_FLOATS",
              "GENPHI_NO_SMALL", "GENPHI_LDS_CAP_FLOATS", "GENPHI_MAX_RUN", "GENPHI_MAX_GROUP"):
        monkeypatch.delenv(k, raising=False)
    # genea140 (real pedigree, kinships down to 2^-35: some rows are not certified), default geometry
    ped = gen.genealogy(gen.genea140)
    gold = np.load(os.path.join(HERE, "golden", "genea140_phi_oracle.npy"))
    for env in ({}, {"GENPHI_NO_FAST": "1"}, {"GENPHI_CERT_MIN_EXP": "-12"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _assert_equal(gen.phi(ped), gold)
        for k in env:
            monkeypatch.delenv(k, raising=False)


def test_rows_of_several_column_chunks(gen, oracle, monkeypatch):
    """Rows wider than one workgroup's columns are cut into column chunks (cfg4's final level: 4 chunks; work
    item = sibling group x chunk).  Forced here on 6500 probands by the columns-per-thread hook, so that every
    level has 2 chunks: certified and mixed levels, the grouping-exact kernel alone, 512- and 1024-thread
    variants, row shards -- all bit-equal to the oracle."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(30000, 6500, 5, skip_permille=20)
    want = oracle.Pedigree(ind, fa, mo).phi(pro)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    knobs = ("GENPHI_FAST_NT", "GENPHI_MAX_CPT", "GENPHI_CERT_MIN_EXP", "GENPHI_NO_FAST")
    monkeypatch.setenv("GENPHI_FULL_MAX_FLOATS", "0")                      # every level is SPLIT
    for env in ({"GENPHI_MAX_CPT": "4"},
                {"GENPHI_MAX_CPT": "4", "GENPHI_FAST_NT": "512"},
                {"GENPHI_MAX_CPT": "4", "GENPHI_FAST_NT": "512", "GENPHI_CERT_MIN_EXP": "-6"},
                {"GENPHI_MAX_CPT": "4", "GENPHI_CERT_MIN_EXP": "-4"},
                {"GENPHI_MAX_CPT": "4", "GENPHI_NO_FAST": "1"}):
        for k in knobs:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        pl = gen.plan(ped, pro)
        assert set(pl.step_modes()) == {1}
        _assert_equal(pl.compute(), want)
        n = len(want)
        parts = [pl.compute(rows=r) for r in [(0, 1000), (1000, 1001), (1001, n)]]
        _assert_equal(np.concatenate(parts, axis=0), want)
        pl.close()
    for k in knobs + ("GENPHI_FULL_MAX_FLOATS",):
        monkeypatch.delenv(k, raising=False)


def test_graph_replay_survives_shard_changes_and_release(gen, oracle):
    """A captured hipGraph bakes device pointers in; every reallocation (another shard, a larger
    result) must retire it.  Sequence A, A, B, A, A with a larger shard B in between, then a
    release of all device memory and a re-upload."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.deep_inbred(40, 40, 3)                   # 39 level steps: graphs are used (>= 8)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    want = oracle.Pedigree(ind, fa, mo).phi(pro)
    pl = gen.plan(ped, pro)
    A, B = (3, 11), (0, 40)
    for r in (A, A, A, B, A, A, A, B, B, B, A):
        _assert_equal(pl.compute(rows=r), want[r[0]:r[1]])
    _assert_equal(pl.compute(), want)
    pl.release_device()
    for r in (A, A, A, None, None, None):
        got = pl.compute(rows=r)
        _assert_equal(got, want if r is None else want[r[0]:r[1]])
    pl.release_device()
    pl.release_device()                                                    # idempotent
    _assert_equal(pl.compute(device=0), want)
    pl.close()


def test_wide_levels_block_assembly(gen, oracle, monkeypatch):
    """WIDE steps (a source row does not fit in LDS; forced here by shrinking the LDS budget): the
    level is assembled from row compaction (dragged x dragged, new x dragged), a transpose (dragged x
    new) and a FULL / SPLIT sub-step on the compacted parent matrix (new x new) -- or the per-entry
    kernel when the parents are too many as well; with few dragged members the dragged rows come whole
    from drag_rows_kernel and the transpose runs the other way (both routes forced here).  Overlapping generations (most of a cut is dragged
    along), a WIDE last step (proband-order delivery), row shards, certificates on and off."""
    from genlib_jl_amd import synth
    seen_nn = set()
    for cap, fullmax, args, kw in [(3200, 8192, (16000, 400, 16), dict(skip_permille=600)),       # new x new by a FULL sub-step
                                   (1500, 8192, (9000, 600, 10), dict(skip_permille=400)),
                                   (1500, 0, (9000, 600, 10), dict(skip_permille=400)),
                                   (700, 8192, (9000, 600, 10), dict(skip_permille=400, seed=5)),
                                   (400, 8192, (4000, 900, 6), dict(skip_permille=150)),        # last step WIDE too
                                   (256, 8192, (3000, 300, 12), dict(skip_permille=100, seed=11))]:
        monkeypatch.setenv("GENPHI_LDS_CAP_FLOATS", str(cap))
        monkeypatch.setenv("GENPHI_FULL_MAX_FLOATS", str(fullmax))
        ind, fa, mo, sex, pro = synth.random_mating(*args, **kw)
        ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
        want = oracle.Pedigree(ind, fa, mo).phi(pro)
        for env in ({}, {"GENPHI_NO_FAST": "1"}, {"GENPHI_CERT_MIN_EXP": "-5"}, {"GENPHI_WIDE_ROUTE": "A"},
                    {"GENPHI_WIDE_ROUTE": "B", "GENPHI_CERT_MIN_EXP": "-5"}):
            for k in ("GENPHI_NO_FAST", "GENPHI_CERT_MIN_EXP", "GENPHI_WIDE_ROUTE"):
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            pl = gen.plan(ped, pro)
            modes = pl.step_modes()
            assert 2 in modes
            seen_nn |= {pl.step_info(k)[3] for k in range(len(modes)) if modes[k] == 2}
            _assert_equal(pl.compute(), want)
            _assert_equal(pl.compute(kernel=1), want)
            n = len(want)
            parts = [pl.compute(rows=r) for r in [(0, 7), (7, n // 2), (n // 2, n)]]
            _assert_equal(np.concatenate(parts, axis=0), want)
            pl.close()
    assert {0, 1, 3} <= seen_nn, seen_nn          # FULL, SPLIT and per-entry new x new blocks all exercised
    for k in ("GENPHI_NO_FAST", "GENPHI_CERT_MIN_EXP", "GENPHI_LDS_CAP_FLOATS", "GENPHI_FULL_MAX_FLOATS", "GENPHI_WIDE_ROUTE"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.gpu
def test_wide_levels_stay_in_place(gen, oracle, monkeypatch):
    """Persistent slots (csrc/planner.h LevelStep::stay): in a run of WIDE steps the members keep their row / column of ONE
    level matrix, the dragged x dragged block (src/compute.jl:108-110) is never copied, new members take the slots of members
    that left the cuts.  Forced here by a small LDS budget on overlapping-generation pedigrees: growing and shrinking cuts, runs
    that wrap around the slot space, the step that leaves a run (reads by slot, writes compactly), certificates on and off
    (the grouping-exact kernels), repeated sweeps on one plan (dead slots keep stale values), the captured-graph replay, the
    per-entry kernel sweep on the same plan (no slots), row shards; == the oracle, and == the same plan without in-place steps."""
    from genlib_jl_amd import synth
    stays = 0
    # (cuts wider than the LDS budget whose new members' parents fit in it: the new x new block has a row kernel)
    for cap, args, kw in [(3000, (20000, 300, 18), dict(skip_permille=500, seed=2)),
                          (2000, (30000, 400, 30), dict(skip_permille=600, seed=3)),
                          (1200, (12000, 500, 24), dict(skip_permille=700, seed=8)),
                          (900, (8000, 300, 20), dict(skip_permille=800, seed=21)),
                          (64, (1046, 388, 15), dict(skip_permille=150, seed=213737704)),      # tiny cuts: < 64 new members per step, steps
                          (64, (786, 255, 10), dict(skip_permille=30, seed=499794305))]:       # next to the fused small-level run
        ind, fa, mo, sex, pro = synth.random_mating(*args, **kw)
        ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
        want = oracle.Pedigree(ind, fa, mo).phi(pro)
        for env in ({}, {"GENPHI_CERT_MIN_EXP": "-4"}, {"GENPHI_NO_FAST": "1"}, {"GENPHI_STAY_HEADROOM": "3"},
                    {"GENPHI_STAY_HEADROOM": "2", "GENPHI_CERT_MIN_EXP": "-4"}, {"GENPHI_STAY_SCATTER": "1"}, {"GENPHI_STAY_TWO_PASS": "1", "GENPHI_CERT_MIN_EXP": "-6"},
                    {"GENPHI_NO_STAY": "1"}):
            for k in ("GENPHI_CERT_MIN_EXP", "GENPHI_NO_FAST", "GENPHI_NO_STAY", "GENPHI_STAY_HEADROOM", "GENPHI_STAY_SCATTER", "GENPHI_STAY_TWO_PASS"):
                monkeypatch.delenv(k, raising=False)
            monkeypatch.setenv("GENPHI_LDS_CAP_FLOATS", str(cap))
            monkeypatch.setenv("GENPHI_STAY_MEM_PCT", "1000")      # (small cuts: the slot matrix may exceed 1.2 x the plain buffers)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            pl = gen.plan(ped, pro)
            n_steps = len(pl.step_modes())
            flags = [pl.step_slots(k) for k in range(n_steps)]
            n_stay = sum(f[0] & 1 for f in flags)
            if "GENPHI_NO_STAY" in env:
                assert n_stay == 0 and all(f == (0, 0, 0, 0) for f in flags)
            else:
                assert n_stay >= 2 or cap == 64, flags
                stays += n_stay
                for k, f in enumerate(flags):
                    if f[0] & 1:                     # in place: reads and writes by slot, the next step reads by slot too
                        assert f[0] & 2 and (k + 1 == len(flags) or flags[k + 1][0] & 2) and f[2] % 64 == 0 and f[3] % 64 == 0 and f[2] < f[1]      # (the proband step may stay in place too)
            for rep in range(4):                     # (the 3rd and 4th call of a >= 8-step sweep replay the captured graph)
                _assert_equal(pl.compute(), want)
            _assert_equal(pl.compute(kernel=1), want)
            _assert_equal(pl.compute(), want)
            n = len(want)
            parts = [pl.compute(rows=r) for r in [(0, 5), (5, n // 3), (n // 3, n)]]
            _assert_equal(np.concatenate(parts, axis=0), want)
            if not env and cap == 3000:
                # the Float64 sweep on the same plan knows no slots (compact index arrays, its own buffers with the run's pitch)
                pl.compute_device(storage64=True)
                m64 = pl.result_to_host_f64()
                pl.compute_device(storage64=True, kernel=1)
                assert np.array_equal(m64, pl.result_to_host_f64())                  # row-staged == per-entry Float64 kernel
                # (against the Float32-per-level result: one rounding per level apart; the exact recursion is exponential at this depth)
                assert np.array_equal(m64, m64.T) and np.abs(m64 - want.astype(np.float64)).max() < 1e-6
                _assert_equal(pl.compute(), want)
            pl.close()
    assert stays >= 100
    # a real genealogy (irregular generation gaps: members of one block leave at many different steps), wide levels forced
    ped = gen.genealogy(gen.genea140)
    pro = gen.pro(ped)
    want = oracle.Pedigree.from_file(gen.genea140).phi(pro)
    for k in ("GENPHI_CERT_MIN_EXP", "GENPHI_NO_FAST", "GENPHI_NO_STAY", "GENPHI_STAY_HEADROOM", "GENPHI_STAY_SCATTER"):
        monkeypatch.delenv(k, raising=False)
    for cap in (8000, 4000):
        monkeypatch.setenv("GENPHI_LDS_CAP_FLOATS", str(cap))
        pl = gen.plan(ped, pro)
        assert sum(pl.step_slots(k)[0] & 1 for k in range(len(pl.step_modes()))) >= 1
        _assert_equal(pl.compute(), want)
        _assert_equal(pl.compute(), want)
        pl.close()
    for k in ("GENPHI_CERT_MIN_EXP", "GENPHI_NO_FAST", "GENPHI_NO_STAY", "GENPHI_LDS_CAP_FLOATS", "GENPHI_STAY_HEADROOM", "GENPHI_STAY_MEM_PCT", "GENPHI_STAY_SCATTER", "GENPHI_STAY_TWO_PASS"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.gpu
def test_cfg3s_full_size_bit_exact(gen, oracle, monkeypatch):
    """cfg3 as SURVEY.md 8(d) words it -- 5 % of the parents from generation g-2 "to exercise the dragged path" (1e5 individuals /
    1e4 probands / 20 generations: cuts to 20,540 members, up to 91 % of a cut dragged along, B = 26.25 GB, 55 % of it dragged x
    dragged copies, src/compute.jl:108-110) -- at FULL size against the oracle (1.66e9 pair evaluations), bit for bit, default
    settings: the planner keeps a run of 11 cuts of SPLIT width in place (persistent slots, block assembly).  Also: the same
    pedigree with nothing in place (GENPHI_STAY_NARROW=0: the round-3 plan, every level through the row kernels), the per-entry
    kernel, row shards, the captured-graph replay."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(100_000, 10_000, 20, skip_permille=50)
    want = oracle.Pedigree(ind, fa, mo).phi(pro)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    sizes, both = pl.levels()
    modes = pl.step_modes()
    flags = [pl.step_slots(k) for k in range(len(modes))]
    stay = [k for k, f in enumerate(flags) if f[0] & 1]
    assert max(sizes) == 20_540 and len(stay) >= 10 and all(modes[k] == 2 and sizes[k] <= 36_863 for k in stay)
    assert modes[-1] != 2                                           # the proband step keeps its row kernel (and its row shards)
    for rep in range(4):                                             # eager, eager, captured, replayed
        _assert_equal(pl.compute(), want)
    _assert_equal(pl.compute(kernel=1), want)
    parts = [pl.compute(rows=r) for r in [(0, 3), (3, 4_000), (4_000, 10_000)]]
    _assert_equal(np.concatenate(parts, axis=0), want)
    pl.close()
    assert np.array_equal(want, want.T)
    monkeypatch.setenv("GENPHI_STAY_NARROW", "0")
    pl = gen.plan(ped, pro)
    assert 2 not in pl.step_modes() and all(pl.step_slots(k) == (0, 0, 0, 0) for k in range(len(modes)))
    _assert_equal(pl.compute(), want)
    pl.close()
    monkeypatch.delenv("GENPHI_STAY_NARROW", raising=False)


@pytest.mark.gpu
def test_narrow_levels_stay_in_place(gen, oracle, monkeypatch):
    """Persistent slots at FULL / SPLIT widths (round 4): the variants of test_wide_levels_stay_in_place on plans whose source rows
    FIT in LDS -- default LDS budget, the steps are switched to block assembly by the planner's cost model, not by their width.
    Growing and shrinking cuts, runs that wrap around the slot space and runs the slot space ends early, the step that leaves a run,
    the entry cut written by the 1/2 I kernel / a FULL step / a fused small-level run, certificates on and off, the scatter buffer,
    the two-pass form, repeated sweeps and the graph replay, the per-entry kernel sweep on the same plan, row shards, the Float64
    sweep; == the oracle and == the plan with nothing in place."""
    from genlib_jl_amd import synth
    stays = 0
    for nmin, args, kw in [(2048, (20000, 300, 18), dict(skip_permille=500, seed=2)),
                           (2048, (30000, 400, 30), dict(skip_permille=600, seed=3)),
                           (64, (12000, 500, 24), dict(skip_permille=700, seed=8)),
                           (64, (8000, 300, 20), dict(skip_permille=800, seed=21)),
                           (2048, (60000, 3000, 12), dict(skip_permille=100, seed=5)),
                           (0, (1046, 388, 15), dict(skip_permille=150, seed=213737704)),
                           (0, (786, 255, 10), dict(skip_permille=30, seed=499794305))]:
        ind, fa, mo, sex, pro = synth.random_mating(*args, **kw)
        ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
        want = oracle.Pedigree(ind, fa, mo).phi(pro)
        knobs = ("GENPHI_CERT_MIN_EXP", "GENPHI_NO_FAST", "GENPHI_NO_STAY", "GENPHI_STAY_HEADROOM", "GENPHI_STAY_SCATTER", "GENPHI_STAY_TWO_PASS",
                 "GENPHI_STAY_NARROW", "GENPHI_STAY_SLACK_PCT", "GENPHI_FULL_MAX_FLOATS", "GENPHI_STAY_SCALAR_T")
        for env in ({}, {"GENPHI_CERT_MIN_EXP": "-4"}, {"GENPHI_NO_FAST": "1"}, {"GENPHI_STAY_HEADROOM": "2", "GENPHI_CERT_MIN_EXP": "-4"},
                    {"GENPHI_STAY_SCATTER": "1"}, {"GENPHI_STAY_TWO_PASS": "1", "GENPHI_CERT_MIN_EXP": "-6"}, {"GENPHI_STAY_SLACK_PCT": "0"},
                    {"GENPHI_FULL_MAX_FLOATS": "0"}, {"GENPHI_STAY_SCALAR_T": "1"}, {"GENPHI_STAY_NARROW": "0"}):
            for k in knobs:
                monkeypatch.delenv(k, raising=False)
            monkeypatch.setenv("GENPHI_STAY_NARROW_MIN", str(nmin))
            monkeypatch.setenv("GENPHI_STAY_OVERHEAD_K", "0")      # (bytes only: the launch overhead term would keep these small cuts on their row kernels)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            pl = gen.plan(ped, pro)
            sizes, both = pl.levels()
            modes = pl.step_modes()
            flags = [pl.step_slots(k) for k in range(len(modes))]
            n_stay = sum(f[0] & 1 for f in flags)
            if "GENPHI_STAY_NARROW" in env:
                assert n_stay == 0 and 2 not in modes
            else:
                assert n_stay >= 3, (args, env, flags)
                stays += n_stay
                for k, f in enumerate(flags):
                    if f[0] & 1:                     # in place: block assembly although a source row fits in LDS; the next step reads by slot
                        assert modes[k] == 2 and sizes[k] <= 36_863 and f[0] & 2 and (k + 1 == len(flags) or (flags[k + 1][0] & 2 and modes[k + 1] == 2))
                assert modes[-1] != 2 or flags[-1][0] & 1      # (the proband step: a row kernel, or in place at the end of a run)
            for rep in range(4):
                _assert_equal(pl.compute(), want)
            _assert_equal(pl.compute(kernel=1), want)
            _assert_equal(pl.compute(), want)
            n = len(want)
            parts = [pl.compute(rows=r) for r in [(0, 5), (5, n // 3), (n // 3, n)]]
            _assert_equal(np.concatenate(parts, axis=0), want)
            if not env and args[0] == 20000:
                pl.compute_device(storage64=True)
                m64 = pl.result_to_host_f64()
                pl.compute_device(storage64=True, kernel=1)
                assert np.array_equal(m64, pl.result_to_host_f64())
                assert np.array_equal(m64, m64.T) and np.abs(m64 - want.astype(np.float64)).max() < 1e-6
                _assert_equal(pl.compute(), want)
            pl.close()
    assert stays >= 300
    for k in knobs + ("GENPHI_STAY_NARROW_MIN", "GENPHI_STAY_OVERHEAD_K"):
        monkeypatch.delenv(k, raising=False)
    # a real genealogy: the cost model keeps genea140's row kernels (36-46 % of the members of its wide cuts are new); lowering
    # the bar (a cut needs only 110 % of its new members) does not change that -- forced in place through the LDS budget instead
    # in test_wide_levels_stay_in_place
    ped = gen.genealogy(gen.genea140)
    pl = gen.plan(ped, gen.pro(ped))
    assert 2 not in pl.step_modes()
    pl.close()


def test_pairwise_phi_float64(gen, oracle):
    """gen.phi(individual_i, individual_j) (src/compute.jl:66-95): Float64 kinship of a pair from one
    Float64 level sweep.  Reference pins: test/runtests.jl:49 (phi(ped[1], ped[2]) == 0.37109375) and
    :58-60 (two founders -> 0); everything else against the oracle's literal recursion, bit for bit
    (tolerance of the north star: 1e-12; asserted: 0)."""
    ped = gen.genealogy(gen.geneaJi)
    assert gen.phi(ped[1], ped[2]) == GOLD["geneaJi"]["phi_pair_1_2"]
    founders = gen.founder(ped)
    assert gen.phi(ped[int(founders[0])], ped[int(founders[1])]) == 0.0
    assert isinstance(gen.phi(ped[1], ped[2]), float)
    op = oracle.Pedigree.from_file(gen.geneaJi)
    for i in ped.ind:
        for j in ped.ind[::3]:
            assert gen.phi(ped[int(i)], ped[int(j)]) == op.phi_pair(int(i), int(j)), (i, j)
    assert gen.phi(ped[1], ped[1]) == 0.5 + 0.5 * op.phi_pair(int(ped[1].father.ID), int(ped[1].mother.ID))
    with pytest.raises(KeyError):
        ped[424242]
    assert ped[1].father.ID == int(ped.father[ped.positions([1])[0]]) and ped[int(founders[0])].father is None
    # many pairs in one sweep through the C-ABI (genphi_phi_pairs), genea140
    from genlib_jl_amd import _capi
    ped = gen.genealogy(gen.genea140)
    op = oracle.Pedigree.from_file(gen.genea140)
    pro = gen.pro(ped)
    rng = np.random.default_rng(1)
    a = rng.choice(pro, 24); b = rng.choice(pro, 24)
    a[3] = b[3]                                                            # a self pair
    got = _capi.phi_pairs(ped.ind, ped.father, ped.mother, a, b)
    want = np.array([op.phi_pair(int(x), int(y)) for x, y in zip(a, b)])
    assert got.dtype == np.float64 and np.array_equal(got, want), np.abs(got - want).max()
    assert np.count_nonzero(got) > 5
    # the Float64 result of a plan: all rows, shards, and its Float32 delivery (one rounding)
    sub = pro[:30]
    pl = gen.plan(ped, sub)
    pl.compute_device(storage64=True)
    full = pl.result_to_host_f64()
    want = np.array([[op.phi_pair(int(x), int(y)) for y in sub[:6]] for x in sub[:6]])
    assert np.array_equal(full[:6, :6], want) and np.array_equal(full, full.T)
    assert np.array_equal(pl.result_to_host(), full.astype(np.float32))
    pl.compute_device(storage64=True, rows=(4, 9))
    assert np.array_equal(pl.result_to_host_f64(), full[4:9])
    assert np.array_equal(pl.result_entries([4, 8], [0, 29]), full[[4, 8], [0, 29]])
    pl.compute_device()                                                    # back to the Float32 sweep on the same plan
    _assert_equal(pl.result_to_host(), oracle.Pedigree.from_file(gen.genea140).phi(sub))
    pl.close()


@pytest.mark.gpu
def test_float64_sweep_kernels(gen, oracle, monkeypatch):
    """The Float64 level sweep (GENPHI_FLAG_STORAGE_F64; src/compute.jl:66-95 arithmetic): the persistent row-staged
    kernel (level_full64_kernel: column index words in registers, next row pair in flight) against the per-entry
    kernel on the same plans -- every block size, several column chunks, a final level kept in [dragged, new] order
    (forced WIDE plan: colmap), row shards -- and against the oracle's literal pairwise recursion on samples."""
    from genlib_jl_amd import synth
    rng = np.random.default_rng(11)

    def both(ind, fa, mo, pro, samples, rows=None):
        ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)})
        pl = gen.plan(ped, pro)
        pl.compute_device(storage64=True, rows=rows)
        a = pl.result_to_host_f64().copy()
        pl.compute_device(storage64=True, kernel=1, rows=rows)
        b = pl.result_to_host_f64()
        assert a.dtype == np.float64 and np.array_equal(a, b), np.abs(a - b).max()
        r0 = rows[0] if rows else 0
        op = oracle.Pedigree(ped.ind, ped.father, ped.mother)
        for i, j in samples:
            if r0 <= i < r0 + a.shape[0]:
                assert a[i - r0, j] == op.phi_pair(int(pro[i]), int(pro[j])), (i, j)
        pl.close()
        return a

    # (a) overlapping generations (dragged members, one-parent rows), cuts of a few thousand: 256- and 512-thread workgroups
    ind, fa, mo, sex, pro = synth.random_mating(20000, 1500, 8, skip_permille=100, seed=5)
    sm = [(int(x), int(y)) for x, y in zip(rng.integers(0, 1500, 12), rng.integers(0, 1500, 12))] + [(7, 7)]
    full = both(ind, fa, mo, pro, sm)
    assert np.array_equal(full, full.T) and np.count_nonzero(full) > 1500
    part = both(ind, fa, mo, pro, sm, rows=(700, 1100))
    assert np.array_equal(part, full[700:1100])
    # (b) the same through a plan whose last step is WIDE: the last cut stays in [dragged, new] order (colmap)
    monkeypatch.setenv("GENPHI_LDS_CAP_FLOATS", "1024")
    monkeypatch.setenv("GENPHI_NO_SMALL", "1")
    wide = both(ind, fa, mo, pro, sm[:4])
    assert np.array_equal(wide, full)
    monkeypatch.delenv("GENPHI_LDS_CAP_FLOATS"); monkeypatch.delenv("GENPHI_NO_SMALL")
    # (c) an output far wider than the cut above it: 11 000 probands from 60 parents -> two column chunks of 512 x 20
    n_par, n_pro = 60, 11000
    ind = np.arange(1, n_par + n_pro + 1, dtype=np.int64)
    fa = np.zeros(len(ind), dtype=np.int64); mo = np.zeros(len(ind), dtype=np.int64)
    fa[n_par:] = 1 + 2 * rng.integers(0, n_par // 2, n_pro)
    mo[n_par:] = 2 + 2 * rng.integers(0, n_par // 2, n_pro)
    mo[n_par + 5] = 0                                              # a one-parent proband
    pro = ind[n_par:]
    sm = [(int(x), int(y)) for x, y in zip(rng.integers(0, n_pro, 10), rng.integers(0, n_pro, 10))] + [(10500, 10999), (10999, 10999), (5, 5)]
    got = both(ind, fa, mo, pro, sm)
    assert got.shape == (n_pro, n_pro) and np.array_equal(got[:300, 10240:], got[10240:, :300].T)
    # (e) cuts between 10,240 and 20,479 members: one Float64 row at a time in LDS (level_split64_kernel), genea140's widest levels
    ped = gen.genealogy(gen.genea140)
    op = oracle.Pedigree.from_file(gen.genea140)
    pro = gen.pro(ped)
    pl = gen.plan(ped, pro)
    assert max(pl.levels()[0]) > 10240
    pl.compute_device(storage64=True)
    a = pl.result_to_host_f64().copy()
    pl.compute_device(storage64=True, kernel=1)
    assert np.array_equal(a, pl.result_to_host_f64()) and np.array_equal(a, a.T)
    for i, j in [(0, 0), (3, 77), (139, 12), (50, 51)]:
        assert a[i, j] == op.phi_pair(int(pro[i]), int(pro[j])), (i, j)
    pl.compute_device(storage64=True, rows=(20, 61))
    assert np.array_equal(pl.result_to_host_f64(), a[20:61])
    pl.close()
    # (d) tiny cuts: 64-thread workgroups (geneaJi, every individual a proband of its own sweep)
    ped = gen.genealogy(gen.geneaJi)
    op = oracle.Pedigree.from_file(gen.geneaJi)
    pl = gen.plan(ped, ped.ind[-9:])
    pl.compute_device(storage64=True)
    m = pl.result_to_host_f64()
    want = np.array([[op.phi_pair(int(x), int(y)) for y in ped.ind[-9:]] for x in ped.ind[-9:]])
    assert np.array_equal(m, want)
    pl.close()


def test_branching_then_phi(gen, oracle):
    """SURVEY 8(f) row 2 through the GPU: pruning the pedigree to the probands' ancestors
    (gen.branching, src/extract.jl:65-186) must not change gen.phi."""
    ped = gen.genealogy(gen.genea140)
    pro = gen.pro(ped)[10:60]
    pruned = gen.branching(ped, pro=pro)
    assert len(pruned) < len(ped)
    want = oracle.Pedigree.from_file(gen.genea140).phi(pro)
    _assert_equal(gen.phi(pruned, pro), want)
    _assert_equal(gen.phi(ped, pro), want)
    ped = gen.genealogy(gen.geneaJi)
    wantj = oracle.Pedigree.from_file(gen.geneaJi).phi([1, 29])
    _assert_equal(gen.phi(gen.branching(ped, pro=[1, 29]), [1, 29]), wantj)
    _assert_equal(gen.phi(ped, [1, 29]), wantj)


def _sparse_check(gen, oracle, ind, fa, mo, sex, pro, sort=True):
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}, sort=sort)
    K = gen.sparse_phi(ped, pro)
    oped = oracle.Pedigree(ind, fa, mo, sort=sort)
    want = oracle.SparsePhi(oped, pro)
    upro = list(dict.fromkeys(int(x) for x in pro))
    a = np.repeat(upro, len(upro)); b = np.tile(upro, len(upro))
    got = K.get(a, b).reshape(len(upro), len(upro)).astype(np.float32)
    ref = np.array([[want[(x, y)] for y in upro] for x in upro], dtype=np.float32)
    _assert_equal(got, ref)
    nr, nz, sa, sd = K.info()
    wr, wz, wa, wd = want.info()
    assert (nr, nz) == (wr, wz), (nr, nz, wr, wz)
    assert abs(sa - wa) <= 1e-12 * max(1.0, abs(wa)) and abs(sd - wd) <= 1e-12 * max(1.0, abs(wd))
    assert repr(K) == want.show()
    ge, we = K.entries(), want.entries()
    assert sorted(zip(ge[0].tolist(), ge[1].tolist(), ge[2].tolist())) == sorted(zip(we[0].tolist(), we[1].tolist(), we[2].tolist()))
    if nr > 1:
        assert gen.phiMean(K) == want.phi_mean()
    return K, want


def test_sparse_phi_kinship_matrix(gen, oracle):
    """gen.sparse_phi / KinshipMatrix (src/compute.jl:321-447, :31-46, :467-472) on the
    GPU (one depth at a time on a dense active matrix) against the literal restatement in
    oracle/sparse_oracle.cpp: getindex for every pair, the `show` line, phiMean, the stored entries."""
    ped = gen.genealogy(gen.geneaJi)
    K = gen.sparse_phi(ped)
    assert float(gen.phiMean(K)) == 0.171875                              # test/runtests.jl:55
    assert K[1, 2] == 0.37109375                                          # :56
    assert repr(K) == "3×3 KinshipMatrix with 6 stored entries."          # :57
    with pytest.raises(KeyError):
        K[1, 17]
    with pytest.raises(KeyError):
        gen.sparse_phi(ped, [424242])
    from genlib_jl_amd import synth
    oj = oracle.read_tsv(gen.geneaJi)
    _sparse_check(gen, oracle, *oj, pro=[1, 2, 29])
    _sparse_check(gen, oracle, *oj, pro=[29, 1, 9, 1, 17])                  # an ancestor and a founder among the probands, a duplicate
    # random pedigrees; file order shuffled inside the generations, so that individuals of one depth
    # leave the queue in another order than their ranks (the reference's key behaviour shows)
    quirk_seen = False
    for args, kw, seed in [((600, 60, 6), dict(skip_permille=100), 1), ((2000, 150, 8), dict(skip_permille=0), 2),
                           ((1500, 100, 12), dict(skip_permille=200, seed=9), 3)]:
        ind, fa, mo, sex, pro = synth.random_mating(*args, **kw)
        rng = np.random.default_rng(seed)
        perm = rng.permutation(len(ind))
        K, want = _sparse_check(gen, oracle, ind[perm], fa[perm], mo[perm], sex[perm], pro)
        full = want.matrix()
        dense = oracle.Pedigree(ind[perm], fa[perm], mo[perm]).phi(pro)
        quirk_seen |= not np.array_equal(full, dense)
        _sparse_check(gen, oracle, ind, fa, mo, sex, pro[::3])
    assert quirk_seen                                                       # at least one case where sparse != dense in the reference
    one = synth.random_mating(900, 80, 7, skip_permille=50, seed=3)
    mo1 = one[2].copy(); mo1[::13] = 0                                      # one-parent individuals
    _sparse_check(gen, oracle, one[0], one[1], mo1, one[3], one[4])
    # genea140, a subset of the probands (the oracle's dictionaries make the full set slow)
    g = oracle.read_tsv(gen.genea140)
    ped = gen.genealogy(gen.genea140)
    _sparse_check(gen, oracle, *g, pro=gen.pro(ped)[:25])


def test_sparse_phi_unsorted_ranks(gen, oracle, capfd):
    """gen.genealogy(...; sort=false) (src/create.jl:131,161): the rank is the file position, so an
    individual of an earlier depth can carry the larger rank.  sparse_phi then (i) finds fewer kinships
    (lookups use (smaller rank, larger rank), stores use (earlier, later): src/compute.jl:366-394) and
    (ii) keeps entries of retired columns in the dictionaries of probands of EARLIER depths
    (:401-430 deletes phi[rank_j][parent] only for rank_j < parent rank).  Every getindex, the `show`
    line, phiMean and the stored entries must equal the literal restatement."""
    from genlib_jl_amd import synth
    # file order P1 P2 S=(P1,P2) F3 x=(S,F3) j=(P1,P2) F4 y=(x,F4); probands j, y.  j leaves the queue in the
    # depth-2 wave, x in the depth-3 wave, rank(x) = 5 < rank(j) = 6: (6, 5) = 0.125 outlives x
    ind = np.arange(1, 9)
    fa = np.array([0, 0, 1, 0, 3, 1, 0, 5]); mo = np.array([0, 0, 2, 0, 4, 2, 0, 7]); sex = np.array([1, 2, 1, 2, 1, 2, 2, 1])
    K, want = _sparse_check(gen, oracle, ind, fa, mo, sex, [6, 8], sort=False)
    assert repr(K) == "2×2 KinshipMatrix with 3 stored entries." and float(gen.phiMean(K)) == 0.125
    assert want.show() == repr(K) and float(want.phi_mean()) == 0.125
    K, _ = _sparse_check(gen, oracle, ind, fa, mo, sex, [6, 8], sort=True)  # depth-sorted ranks: (6, 7) is deleted, Phi(j, y) is found
    assert K[6, 8] == 0.0625 and float(gen.phiMean(K)) == 0.0625
    n_cross = 0
    for args, kw, seed in [((600, 60, 6), dict(skip_permille=100), 1), ((2000, 150, 8), dict(skip_permille=0), 2),
                           ((1500, 100, 12), dict(skip_permille=200, seed=9), 3), ((900, 80, 7), dict(skip_permille=50, seed=3), 4)]:
        ind, fa, mo, sex, pro = synth.random_mating(*args, **kw)
        if seed == 4:
            mo = mo.copy(); mo[::13] = 0                                    # one-parent individuals
        i2, f2, m2, s2 = synth.parents_first_shuffle(ind, fa, mo, sex, seed=seed)
        extra = i2[np.random.default_rng(seed).integers(0, len(i2), 12)]    # ancestors among the probands: earlier depths, any rank
        for p in (pro, np.concatenate([pro[::2], extra])):
            K, want = _sparse_check(gen, oracle, i2, f2, m2, s2, p, sort=False)
            a, b = _sparse_check(gen, oracle, i2, f2, m2, s2, p, sort=True)
            n_cross += K.info()[1] != a.info()[1]
    assert n_cross >= 3                                                     # the file order really changes what is stored
    # more outliving entries than the first sweep's list holds: the sweep runs a second time with the list sized exactly, on the same
    # pool and stream; then ordinary calls again on the device side that call left behind, smaller and larger than it
    ind, fa, mo, sex, pro = synth.random_mating(1500, 100, 12, skip_permille=200, seed=9)
    i2, f2, m2, s2 = synth.parents_first_shuffle(ind, fa, mo, sex, seed=3)
    extra = i2[np.random.default_rng(3).integers(0, len(i2), 12)]
    p = np.concatenate([pro[::2], extra])
    K0, _ = _sparse_check(gen, oracle, i2, f2, m2, s2, p, sort=False)
    os.environ["GENPHI_SPARSE_STALE_CAP"] = "1"
    os.environ["GENPHI_TRACE"] = "1"
    capfd.readouterr()
    try:
        K1, _ = _sparse_check(gen, oracle, i2, f2, m2, s2, p, sort=False)
    finally:
        del os.environ["GENPHI_SPARSE_STALE_CAP"], os.environ["GENPHI_TRACE"]
    assert capfd.readouterr().err.count("sweep done") == 2                  # the list overflowed, the sweep ran twice
    assert K1.info() == K0.info() and all(np.array_equal(x, y) for x, y in zip(K1.entries(), K0.entries()))
    # the other form of a wave: rows + new x new as two kernels with T in HBM (round 3; the default builds a new row end to end in LDS)
    for knob, val in (("GENPHI_SPARSE_NO_FUSED", "1"),):
        os.environ[knob] = val
        try:
            K2, _ = _sparse_check(gen, oracle, i2, f2, m2, s2, p, sort=False)
            assert K2.info() == K0.info() and all(np.array_equal(x, y) for x, y in zip(K2.entries(), K0.entries())), (knob, val)
            one = synth.random_mating(900, 80, 7, skip_permille=50, seed=3)
            mo1 = one[2].copy(); mo1[::13] = 0                              # one-parent individuals
            _sparse_check(gen, oracle, one[0], one[1], mo1, one[3], one[4])
            g = oracle.read_tsv(gen.genea140)
            _sparse_check(gen, oracle, *g, pro=gen.pro(gen.genealogy(gen.genea140))[:25])
        finally:
            del os.environ[knob]
    for args in [(300, 30, 5), (4000, 300, 9), (600, 60, 6), (4000, 300, 9)]:
        q = synth.random_mating(*args, seed=21)
        held = [_sparse_check(gen, oracle, *q[:4], q[4], sort=True)[0] for _ in range(2)]      # two results alive at once: separate host blocks
        assert held[0].info() == held[1].info()
    g = oracle.read_tsv(gen.genea140)                                       # genea140 in its own file order, and shuffled parents-first
    ped = gen.genealogy(gen.genea140, sort=False)
    assert np.array_equal(ped.ind, g[0])
    _sparse_check(gen, oracle, *g, pro=gen.pro(ped)[:25], sort=False)
    g2 = synth.parents_first_shuffle(*g, seed=11)
    _sparse_check(gen, oracle, *g2, pro=gen.pro(ped)[5:30], sort=False)


def test_dense_phi_f_and_pairs_with_unsorted_ranks(gen, oracle, monkeypatch):
    """The same for the dense path: with sort=false the rank (file position) decides which side the
    per-pair kernel climbs first (src/compute.jl:130,139), i.e. the grouping of the Float64 sums.  Every
    kernel family (FULL, SPLIT certified / grouping-exact / mixed, WIDE both routes, SMALL, per-entry,
    identity), row shards, gen.f and the pairwise gen.phi on parents-first files with interleaved depths,
    against the oracle run on the same order."""
    from genlib_jl_amd import synth
    from genlib_jl_amd import _capi
    base = synth.random_mating(5000, 500, 8, skip_permille=60)
    tiny = synth.chain_two_lines(22); tiny2 = synth.chain_two_lines(40)    # kinships 2^-45, 2^-81: rows without a certificate
    knobs = ("GENPHI_FULL_MAX_FLOATS", "GENPHI_LDS_CAP_FLOATS", "GENPHI_NO_FAST", "GENPHI_CERT_MIN_EXP", "GENPHI_WIDE_ROUTE",
             "GENPHI_NO_SMALL", "GENPHI_FAST_NT", "GENPHI_MAX_CPT")
    for case, seed in [(_merge([base, tiny, tiny2]), 1), (synth.random_mating(3000, 300, 12, skip_permille=150, seed=11), 2),
                       (synth.deep_inbred(40, 30, 3), 3)]:
        ind, fa, mo, sex, pro = case
        i2, f2, m2, s2 = synth.parents_first_shuffle(ind, fa, mo, sex, seed=seed)
        if seed == 2:
            m2 = m2.copy(); m2[::17] = 0                                    # one-parent members
        ped = gen.genealogy({"ind": i2, "father": f2, "mother": m2, "sex": s2}, sort=False)
        assert np.array_equal(ped.ind, i2)                                  # the file order IS the rank order
        oped = oracle.Pedigree(i2, f2, m2, sort=False)
        pro = np.concatenate([np.random.default_rng(seed).permutation(pro), i2[:3]])
        want = oped.phi(pro)
        n = len(want)
        for env in ({}, {"GENPHI_NO_SMALL": "1"}, {"GENPHI_FULL_MAX_FLOATS": "0"}, {"GENPHI_FULL_MAX_FLOATS": "0", "GENPHI_NO_FAST": "1"},
                    {"GENPHI_FULL_MAX_FLOATS": "0", "GENPHI_CERT_MIN_EXP": "-6", "GENPHI_LDS_CAP_FLOATS": "1024"},
                    {"GENPHI_FULL_MAX_FLOATS": "0", "GENPHI_FAST_NT": "512", "GENPHI_MAX_CPT": "4", "GENPHI_CERT_MIN_EXP": "-3"},
                    {"GENPHI_LDS_CAP_FLOATS": "300", "GENPHI_WIDE_ROUTE": "A"}, {"GENPHI_LDS_CAP_FLOATS": "300", "GENPHI_WIDE_ROUTE": "B", "GENPHI_NO_FAST": "1"},
                    {"GENPHI_LDS_CAP_FLOATS": "150", "GENPHI_FULL_MAX_FLOATS": "0", "GENPHI_CERT_MIN_EXP": "-8"}):
            for k in knobs:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            pl = gen.plan(ped, pro)
            _assert_equal(pl.compute(), want)
            _assert_equal(np.concatenate([pl.compute(rows=r) for r in [(0, 5), (5, n // 2), (n // 2, n)]], axis=0), want)
            pl.close()
        for k in knobs:
            monkeypatch.delenv(k, raising=False)
        _assert_equal(gen.phi(ped, pro, kernel=1), want)
        if seed != 3:                                                       # (the pairwise recursion is exponential on the inbred lines)
            ids = np.random.default_rng(seed).choice(i2, 40, replace=False)
            assert np.array_equal(gen.f(ped, ids), oped.f(ids))
            a = np.random.default_rng(seed + 7).choice(i2, 16); b = np.random.default_rng(seed + 8).choice(i2, 16)
            got = _capi.phi_pairs(ped.ind, ped.father, ped.mother, a, b)
            assert np.array_equal(got, np.array([oped.phi_pair(int(x), int(y)) for x, y in zip(a, b)]))
    # genea140 in a shuffled parents-first file order (its own file happens to be depth-sorted already)
    g = synth.parents_first_shuffle(*oracle.read_tsv(gen.genea140), seed=5)
    ped = gen.genealogy({"ind": g[0], "father": g[1], "mother": g[2], "sex": g[3]}, sort=False)
    oped = oracle.Pedigree(g[0], g[1], g[2], sort=False)
    _assert_equal(gen.phi(ped), oped.phi())


def test_cfg4o_downscaled_twin(gen, oracle, monkeypatch):
    """The overlapping-generations workload of bench.py (cfg4o: cfg4's generator with 0.5 % of the parents
    drawn from generation g-2) at 1/50 of its size, with the LDS budget scaled so that the planner picks
    the same kernel families level by level as at full size (SPLIT, 23 x WIDE, 5 x SPLIT): bit-equal to
    the oracle, with the default and with the grouping-exact SPLIT kernels."""
    from genlib_jl_amd import synth
    monkeypatch.setenv("GENPHI_LDS_CAP_FLOATS", "750")
    monkeypatch.setenv("GENPHI_FULL_MAX_FLOATS", "0")
    ind, fa, mo, sex, pro = synth.random_mating(20_000, 2_000, 30, skip_permille=5)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    want = oracle.Pedigree(ind, fa, mo).phi(pro)
    pl = gen.plan(ped, pro)
    assert pl.step_modes() == [1] + [2] * 23 + [1] * 5                   # cfg4o's own sequence (profiles/r02_bench_cfg4o.json)
    sizes, both = pl.levels()
    assert max(sizes) > 2300 and max(b / s for b, s in zip(both, sizes[1:])) > 0.75      # most of a cut is dragged along
    for _ in range(4):                                                   # eager, hipGraph capture, two replays (29 level steps)
        _assert_equal(pl.compute(), want)
    _assert_equal(pl.compute(rows=(100, 900)), want[100:900])            # a WIDE plan with a row shard, then the full sweep again
    _assert_equal(pl.compute(), want)
    pl.close()
    monkeypatch.setenv("GENPHI_NO_FAST", "1")
    pl = gen.plan(ped, pro)
    _assert_equal(pl.compute(), want)
    pl.close()
    for k in ("GENPHI_LDS_CAP_FLOATS", "GENPHI_FULL_MAX_FLOATS", "GENPHI_NO_FAST"):
        monkeypatch.delenv(k, raising=False)


def test_failed_upload_leaves_a_clean_plan(gen, oracle, monkeypatch):
    """Out of memory in the middle of an upload (the expected failure of large plans and of the capacity
    path): the call fails loudly, the plan / panel handle is back in the never-uploaded state (no
    half-allocated buffers behind an 'already on device' flag), and a retry uploads from scratch and
    gives the oracle's matrix.  GENPHI_TEST_FAIL_ALLOC = k makes the k-th device allocation fail."""
    from genlib_jl_amd import synth, _capi
    ind, fa, mo, sex, pro = synth.random_mating(3000, 300, 8, skip_permille=100)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    want = oracle.Pedigree(ind, fa, mo).phi(pro)
    for wide in (False, True):
        if wide:
            monkeypatch.setenv("GENPHI_LDS_CAP_FLOATS", "300")             # WIDE steps: psi_p and its certificates are allocated too
        for k in range(1, 12):
            monkeypatch.setenv("GENPHI_TEST_FAIL_ALLOC", str(k))
            pl = gen.plan(ped, pro)
            failed = False
            try:
                got = pl.compute()
            except gen.GenphiDeviceError:
                failed = True
                got = pl.compute()                                        # the retry starts from scratch
            _assert_equal(got, want)
            pl.close()
            if not failed:
                assert k > 6                                              # fewer allocations than k: nothing to inject
                break
        monkeypatch.delenv("GENPHI_LDS_CAP_FLOATS", raising=False)
    for k in (1, 2, 5):
        monkeypatch.setenv("GENPHI_TEST_FAIL_ALLOC", str(k))
        pp = _capi.PanelPlan(ped.ind, ped.father, ped.mother, np.asarray(pro, dtype=np.int64), 0, 1)
        with pytest.raises(gen.GenphiDeviceError):
            pp.begin()
        pp.begin()                                                        # second attempt: clean upload
        for step in range(pp.n_steps):
            pp.pack(step, 0)
            pp.compute(step, 0)
        _assert_equal(pp.result_to_host(), want)
        pp.close()
    monkeypatch.delenv("GENPHI_TEST_FAIL_ALLOC", raising=False)


def _random_mixed_pedigree(rng, n_gen, per_gen, p_one_parent=0.1, p_skip=0.2, p_founder=0.05):
    """Generations with parents from g-1 or g-2, one-parent members and late founders."""
    ind, fa, mo, gens, nxt = [], [], [], [], 1
    for g in range(n_gen):
        ids = list(range(nxt, nxt + per_gen)); nxt += per_gen
        for x in ids:
            f = m = 0
            if g > 0 and rng.random() >= p_founder:
                gf = g - 2 if (g >= 2 and rng.random() < p_skip) else g - 1
                gm = g - 2 if (g >= 2 and rng.random() < p_skip) else g - 1
                f = int(rng.choice(gens[gf][0::2])); m = int(rng.choice(gens[gm][1::2]))
                u = rng.random()
                if u < p_one_parent / 2:
                    f = 0
                elif u < p_one_parent:
                    m = 0
            ind.append(x); fa.append(f); mo.append(m)
        gens.append(ids)
    a = lambda v: np.asarray(v, dtype=np.int64)
    return a(ind), a(fa), a(mo), a([1 + (k % 2) for k in range(len(ind))]), a(gens[-1])


def test_sparse_leading_levels(gen, oracle, monkeypatch):
    """The leading cuts of a sweep are kept as lists of their non-zero entries (csrc/sparse_levels.hip; the reference's sparse_phi
    stores only `coefficient > 0.` for the same reason, src/compute.jl:391-394): bit-equal to the oracle and to the same plan run
    densely (GENPHI_FLAG_NO_SPARSE), by calibration and with the last sparse cut forced, with row shards and graph replay."""
    from genlib_jl_amd import synth
    for name in ("GENPHI_SPARSE_K", "GENPHI_SPARSE_MIN_CUT", "GENPHI_SPARSE_PERMILLE", "GENPHI_SPARSE_CHUNK", "GENPHI_SPARSE_ARENA"):
        monkeypatch.delenv(name, raising=False)
    gold = np.load(os.path.join(HERE, "golden", "genea140_phi_oracle.npy"))
    ped = gen.genealogy(gen.genea140)
    # default settings: genea140's wide cuts are 0.2-1.2 % non-zero, so most of its levels run on lists
    pl = gen.plan(ped)
    phi = pl.compute()
    k, nnz = pl.sparse_levels()
    sizes = pl.levels()[0]
    assert k >= 6, (k, nnz)
    assert nnz[0] == sizes[0] and all(0 < nnz[c] <= 0.2 * sizes[c] ** 2 for c in range(1, k + 1)), (nnz, sizes)
    _assert_equal(phi, gold)
    _assert_equal(pl.compute(no_sparse=True), gold)
    _assert_equal(pl.compute(), gold)                               # (second sparse sweep: counters and cursors start again)
    parts = [pl.compute(rows=(a, b)) for a, b in [(0, 70), (70, 71), (71, 140)]]
    _assert_equal(np.concatenate(parts, axis=0), gold)
    for _ in range(3):                                              # graph replay (17 steps)
        pl.compute_device()
    _assert_equal(pl.result_to_host(), gold)
    # the Float64-storage sweep (gen.f, pairwise phi) runs its leading cuts on the same lists and writes its first dense matrix in Float64
    pl.compute_device(storage64=True)
    f64_sparse = pl.result_to_host_f64()
    pl.compute_device(storage64=True, no_sparse=True)
    f64_dense = pl.result_to_host_f64()
    assert np.array_equal(f64_sparse, f64_dense) and np.abs(f64_sparse - gold.astype(np.float64)).max() < 1e-7
    oped = oracle.Pedigree.from_file(gen.genea140)
    pro140 = gen.pro(ped)
    for a_, b_ in ((0, 1), (3, 77), (139, 139), (20, 5)):
        assert f64_sparse[a_, b_] == oped.phi_pair(int(pro140[a_]), int(pro140[b_]))      # the exact Float64 recursion, src/compute.jl:66-95
    pl.close()
    for force in ("1", "4", "9", "11", "-1"):
        monkeypatch.setenv("GENPHI_SPARSE_K", force)
        pl = gen.plan(ped)
        _assert_equal(pl.compute(), gold)
        assert pl.sparse_levels()[0] == {"1": 1, "4": 4, "9": 9, "11": 10, "-1": -1}[force], pl.sparse_levels()      # (cut 11 is the last one exact in integer units)
        pl.close()
    monkeypatch.delenv("GENPHI_SPARSE_K", raising=False)
    # small chunks of the sparse -> dense step: rows of several workgroups; a list step as one launch / as a launch per class of row lengths
    monkeypatch.setenv("GENPHI_SPARSE_CHUNK", "1024")
    _assert_equal(gen.phi(ped), gold)
    monkeypatch.delenv("GENPHI_SPARSE_CHUNK", raising=False)
    for v in ("0", "1"):
        monkeypatch.setenv("GENPHI_SPARSE_CLASSES", v)
        _assert_equal(gen.phi(ped), gold)
    monkeypatch.delenv("GENPHI_SPARSE_CLASSES", raising=False)
    # the row-list arenas start small and the calibration run enlarges them where a cut needs more (genea140's cuts 9 and 10 by default;
    # here from 64 / 5,000 / 300,000 entries on: a leg of the run per enlargement): same cuts, same lists, same matrix
    k_default, nnz_default = k, nnz
    for first in ("64", "5000", "300000"):
        monkeypatch.setenv("GENPHI_SPARSE_ARENA", first)
        pl = gen.plan(ped)
        _assert_equal(pl.compute(), gold)
        assert pl.sparse_levels()[0] == k_default and pl.sparse_levels()[1][:k_default + 1] == nnz_default[:k_default + 1], (first, pl.sparse_levels())
        _assert_equal(pl.compute(), gold)
        pl.compute_device(storage64=True)
        assert np.array_equal(pl.result_to_host_f64(), f64_sparse)
        pl.close()
    monkeypatch.delenv("GENPHI_SPARSE_ARENA", raising=False)
    # random mating (every row of every cut new, no dragged members) and overlapping generations, by calibration
    for args, kw in (((30000, 3000, 10), dict(skip_permille=0)), ((30000, 2000, 14), dict(skip_permille=30))):
        ind, fa, mo, sex, pro = synth.random_mating(*args, **kw)
        ped2 = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
        want = oracle.Pedigree(ind, fa, mo).phi(pro)
        monkeypatch.setenv("GENPHI_STAY_NARROW", "0")              # (in-place runs end the eligible steps early)
        pl = gen.plan(ped2, pro)
        _assert_equal(pl.compute(), want)
        assert pl.sparse_levels()[0] >= 2, pl.sparse_levels()
        _assert_equal(pl.compute(no_sparse=True), want)
        pl.close()
        monkeypatch.delenv("GENPHI_STAY_NARROW", raising=False)
        _assert_equal(gen.phi(ped2, pro), want)
    # small pedigrees with every sparse cut forced: one-parent members, late founders, parents from two generations up,
    # probands that are ancestors of probands; dense (up to 100 % non-zero) "sparse" cuts
    monkeypatch.setenv("GENPHI_SPARSE_K", "11")
    monkeypatch.setenv("GENPHI_SPARSE_MIN_CUT", "0")
    rng = np.random.default_rng(11)
    for case in range(12):
        ind, fa, mo, sex, last = _random_mixed_pedigree(rng, int(rng.integers(3, 16)), int(rng.integers(8, 300)))
        pro = np.unique(np.concatenate([last, rng.choice(ind, size=min(7, len(ind)), replace=False)]))
        ped3 = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
        want = oracle.Pedigree(ind, fa, mo).phi(pro)
        pl = gen.plan(ped3, pro)
        _assert_equal(pl.compute(), want)
        n_steps = len(pl.levels()[0]) - 1
        assert pl.sparse_levels()[0] == min(10, n_steps - 2) or n_steps < 3, (pl.sparse_levels(), n_steps)      # (never the proband step, never beyond cut 11)
        pl.close()
    pedj = gen.genealogy(gen.geneaJi)
    _assert_equal(gen.phi(pedj), np.array(GOLD["geneaJi"]["phi"], dtype=np.float32))
    # sparse cuts that reach into a run of steps that stay in place (persistent slots): the first dense matrix is then written BY SLOT,
    # or compactly as the entry cut of the run, and the in-place steps go on from it
    monkeypatch.setenv("GENPHI_STAY_NARROW_MIN", "0")
    monkeypatch.setenv("GENPHI_STAY_OVERHEAD_K", "0")
    monkeypatch.setenv("GENPHI_STAY_MEM_PCT", "100000")
    n_by_slot = 0
    for args, kw in (((6000, 400, 12), dict(skip_permille=150)), ((9000, 300, 16), dict(skip_permille=400, seed=3)), ((30000, 2000, 14), dict(skip_permille=30))):
        ind, fa, mo, sex, pro = synth.random_mating(*args, **kw)
        ped4 = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
        want = oracle.Pedigree(ind, fa, mo).phi(pro)
        for force in ("1", "2", "3", "5", "8"):
            monkeypatch.setenv("GENPHI_SPARSE_K", force)
            pl = gen.plan(ped4, pro)
            _assert_equal(pl.compute(), want)
            k = pl.sparse_levels()[0]
            n_by_slot += int(k >= 1 and bool(pl.step_slots(k)[0] & 1))        # step k stays in place: cut k + 1 written by slot
            _assert_equal(pl.compute(no_sparse=True), want)
            pl.close()
    assert n_by_slot >= 3, n_by_slot


def test_kept_blocks_respect_their_budget():
    """csrc/devcache.hip in a process of its own (GENPHI_KEEP_MB is read once): with a 64 MB budget the blocks of a released 350 MB plan
    are kept only up to the budget, the oldest making room for the newest, and the next plans compute the same matrix from recycled blocks;
    with a budget of 0 nothing is kept."""
    import subprocess
    import sys
    code = (
        "import os, sys, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "import genlib_jl_amd as gen\n"
        "from genlib_jl_amd import _capi\n"
        "gold = np.load(%r)\n"
        "ped = gen.genealogy(gen.genea140)\n"
        "budget = int(os.environ['GENPHI_KEEP_MB']) << 20\n"
        "for rep in range(3):\n"
        "    pl = gen.plan(ped); phi = pl.compute(); pl.close()\n"
        "    assert np.array_equal(phi, gold), rep\n"
        "    kept = _capi.cached_bytes()\n"
        "    assert kept <= budget, (rep, kept, budget)\n"
        "    assert (kept > 0) == (budget > 0), (rep, kept, budget)\n"
        "_capi.release_cached(); assert _capi.cached_bytes() == 0\n"
        "print('ok', budget)\n"
    ) % (os.path.dirname(HERE), os.path.join(HERE, "golden", "genea140_phi_oracle.npy"))
    for mb in ("64", "0"):
        env = dict(os.environ, GENPHI_KEEP_MB=mb, GENPHI_PLAN_CACHE="0")
        run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
        assert run.returncode == 0 and "ok" in run.stdout, (mb, run.stdout[-500:], run.stderr[-2000:])


def test_stress_cases_that_failed_once(gen, oracle):
    """Cases of tests/stress_random.py that a build of this repository got wrong, replayed with their knobs (the stress run itself is
    not part of the suite).  Round 5: the first sweep after the calibration run of the sparse cuts took cut k's lists from the arena
    although the run had written cut k+2 over them (the Float64 sweep of gen.f and a full sweep, small arenas enlarged cut by cut)."""
    import sys
    sys.path.insert(0, HERE)
    import stress_random
    from genlib_jl_amd import synth
    saved = {k: os.environ.get(k) for k in stress_random.KNOBS}
    try:
        for case in (266205955, 834111418, 399799883, 314969413):
            what, env, shape, _, _ = stress_random.run_case(case, gen, synth, oracle)
            assert not what, (case, shape, env, what)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_plan_memory_estimate_and_kept_blocks(gen):
    """genphi_plan_device_bytes_needed (host only) bounds what a sweep allocates -- slot matrices of in-place runs and a result at the
    run's pitch included (the proband cut of genea140 with a quarter of its individuals as probands stays in place) --, and released
    plans leave their blocks to the next one (genphi_cached_bytes) until genphi_release_cached gives them back."""
    from genlib_jl_amd import _capi
    ped = gen.genealogy(gen.genea140)
    ids = np.sort(np.random.default_rng(7).choice(np.asarray(ped.ind), size=len(ped.ind) // 4, replace=False))
    for pro in (gen.pro(ped), ids):
        pl = gen.plan(ped, pro)
        need = pl.device_bytes_needed
        assert pl.device_bytes == 0
        pl.compute_device()
        have = pl.device_bytes
        assert 0 < have <= need <= 1.5 * have + (3 << 30), (have, need)
        pl.close()
    assert _capi.cached_bytes() > 0 or os.environ.get("GENPHI_KEEP_MB") == "0"      # (the suite is also run with nothing kept)
    _capi.release_cached()
    assert _capi.cached_bytes() == 0
    _assert_equal(gen.phi(ped), np.load(os.path.join(HERE, "golden", "genea140_phi_oracle.npy")))
