"""genphi_result_group_sums / gen.phiMeanGroups on the GPU against tests/group_sums_oracle.py (math.fsum of the blocks of the
host matrix) under the rule derived there: equal where the kinships are dyadic numbers of few bits (geneaJi, synthetic pedigrees
of 10 generations), within gamma(n) of the oracle elsewhere (genea140)."""
import ctypes
import os

import numpy as np
import pytest

import group_sums_oracle as GO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POP140 = os.path.join(ROOT, "tests", "golden", "pop140.csv")
SIZES = {"Gaspesia-Acadian": 20, "Gaspesia-FrenchCanadian": 20, "Gaspesia-Loyalist": 20, "Montreal": 22, "NorthShore": 20,
         "Quebec": 16, "Saguenay": 22}
CAP = 4096


def _check(pl, phi, labels, n_groups, form, exact, row_begin=0):
    """group_sums of the plan's resident rows (phi = those rows on the host) against the oracle; returns the outputs."""
    sums, diag, rows, cols, got_form = pl.group_sums(labels, n_groups)
    ref = GO.group_sums(phi, labels, n_groups, row_begin=row_begin)
    print("G=%d form=%d rows=%d: max |device - fsum| / fsum = %.3g" % (
        n_groups, got_form, len(phi), np.max(np.abs(sums - ref[0]) / np.where(ref[0] > 0, ref[0], 1))))
    assert got_form == form
    lab = np.asarray(labels)
    assert np.array_equal(cols, np.bincount(lab[lab >= 0], minlength=n_groups))
    res = lab[row_begin:row_begin + len(phi)]
    assert np.array_equal(rows, np.bincount(res[res >= 0], minlength=n_groups))
    GO.assert_within_rule(sums, diag, ref, exact=exact)
    return sums, diag, rows, cols


# ---- geneaJi ------------------------------------------------------------------------------------------------------------------

def test_geneaJi_groups(gen):
    ped = gen.genealogy(gen.geneaJi)
    assert gen.pro(ped).tolist() == [1, 2, 29]
    pl = gen.plan(ped)
    try:
        phi = pl.compute(device=0)
        _check(pl, phi, [0, 0, 1], 2, 0, True)                                 # {1, 2} and {29}
        _check(pl, phi, [0, 1, 2], 3, 0, True)                                 # each proband alone
        assert np.float32(pl.phi_mean_groups([0, 0, 0])[0, 0]) == np.float32(0.171875)      # test/runtests.jl:53
        assert pl.phi_mean_groups([0, 0, 0])[0, 0] == np.float64(pl.phi_mean())
        alone = pl.phi_mean_groups([0, 1, 2])
        assert np.all(np.isnan(np.diagonal(alone))) and alone[0, 1] == np.float64(phi[0, 1]) and alone[2, 0] == np.float64(phi[2, 0])
    finally:
        pl.close()
    m = gen.phiMeanGroups(ped, {1: "a", 2: "a", 29: "a"}, device=0)
    assert m.names == ["a"] and m.sizes.tolist() == [3] and np.float32(m.mean[0, 0]) == np.float32(0.171875)
    m = gen.phiMeanGroups(ped, {1: "left", 2: "left", 29: "right"}, device=0)
    assert m.names == ["left", "right"] and m.sizes.tolist() == [2, 1] and m.mean[0, 1] == (phi[0, 2] + np.float64(phi[1, 2])) / 2
    assert "left" in repr(m) and "right" in repr(m)


def test_probands_outside_the_groups_take_part_in_the_sweep(gen):
    ped = gen.genealogy(gen.geneaJi)
    m = gen.phiMeanGroups(ped, {1: "a", 29: "b"}, probandIDs=[29, 2, 1], device=0)
    phi = gen.phi(ped, [1, 29], device=0)
    assert m.names == ["a", "b"] and m.sizes.tolist() == [1, 1] and m.mean[0, 1] == np.float64(phi[0, 1]) and np.isnan(m.mean[0, 0])


# ---- genea140 with pop140.csv ---------------------------------------------------------------------------------------------------

def test_genea140_populations(gen):
    ped = gen.genealogy(gen.genea140)
    pop = gen._pop(POP140)
    m = gen.phiMeanGroups(ped, pop, device=0)
    names, ordered, labels = gen._group_order(pop)
    assert m.names == sorted(SIZES) and m.sizes.tolist() == [SIZES[n] for n in m.names]
    phi = gen.phi(ped, ordered, device=0)
    ref = GO.group_sums(phi, labels, 7)
    mean, bound = GO.mean_table(ref)
    print("genea140 mean table:\n%r\nmax |mean - oracle| = %.3g (bound %.3g)" % (m, np.max(np.abs(m.mean - mean)), np.max(bound)))
    assert np.all(np.abs(m.mean - mean) <= bound)
    # the same through a plan: form 0 in the (population, ID) order
    pl = gen.plan(ped, ordered)
    try:
        pl.compute_device(device=0)
        _check(pl, phi, labels, 7, 0, False)
        assert np.array_equal(pl.phi_mean_groups(labels), m.mean)
    finally:
        pl.close()
    # and in gen.pro order, where the populations interleave: form 1, the same table within the rule
    pro = gen.pro(ped)
    index = {n: k for k, n in enumerate(names)}
    mixed = np.array([index[pop[i]] for i in pro.tolist()], dtype=np.int32)
    assert np.any(np.diff(mixed) < 0)
    pl = gen.plan(ped, pro)
    try:
        phi_pro = pl.compute(device=0)
        sums, diag, rows, cols = _check(pl, phi_pro, mixed, 7, 1, False)
        GO.assert_within_rule(sums, diag, ref)                                  # the blocks hold the same entries in another order
        assert np.all(np.abs(pl.phi_mean_groups(mixed, 7) - mean) <= bound)
    finally:
        pl.close()


# ---- synthetic pedigrees --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def synth_plan(gen):
    """2,500 probands of a 10-generation random-mating pedigree: ld = 2,560 (60 padding columns), three column tiles of 1,024,
    kinships that are multiples of 2^-21 or so (every Float64 partial sum exact)."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(30_000, 2_500, 10, skip_permille=50)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    phi = pl.compute(device=0)
    assert phi.shape == (2500, 2500) and pl.result_device()[1] % 64 == 0 and pl.result_device()[1] > 2500
    yield pl, phi
    pl.close()


def _contiguous_labels(n, g, rng):
    """Every group one run, the groups in a shuffled order; runs of seven unlabelled probands at the start, in the middle and at
    the end; from 7 groups on, at least two empty groups and a group of one member."""
    free = n - 3 * 7
    used = min(g, free // 2)
    if g >= 7:
        used = min(used, g - 2)
    sizes = 1 + rng.multinomial(free - used, np.ones(used) / used)
    if used > 2:
        sizes[0] += sizes[1] - 1
        sizes[1] = 1
    runs = [np.full(s, a) for a, s in zip(rng.permutation(g)[:used], sizes)]
    gap, mid = np.full(7, -1), used // 2
    return np.concatenate([gap] + runs[:mid] + [gap] + runs[mid:] + [gap]).astype(np.int32)


@pytest.mark.parametrize("g", [1, 2, 7, 64, 1000, CAP])
def test_synthetic_contiguous_and_random_labels(synth_plan, g):
    pl, phi = synth_plan
    n = len(phi)
    rng = np.random.default_rng(100 + g)
    lab = _contiguous_labels(n, g, rng)
    assert len(lab) == n and lab[0] == -1 and lab[-1] == -1 and lab.max() < g
    sums, diag, rows, cols = _check(pl, phi, lab, g, 0, True)
    again = pl.group_sums(lab, g)
    assert np.array_equal(again[0].view(np.int64), sums.view(np.int64)) and np.array_equal(again[1].view(np.int64), diag.view(np.int64))
    if g >= 7:
        assert np.any(cols == 0) and np.any(cols == 1)
    mean = pl.phi_mean_groups(lab, g)
    assert np.array_equal(np.isnan(mean), ~(np.where(np.eye(g, dtype=bool), np.outer(cols, cols - 1), np.outer(cols, cols)) > 0))
    ref_mean, bound = GO.mean_table((sums, diag, rows, cols))
    assert np.array_equal(mean, ref_mean, equal_nan=True)
    # any order of the labels, a tenth of the probands in no group
    lab = rng.integers(0, g, n).astype(np.int32)
    lab[rng.random(n) < 0.1] = -1
    sums, diag, _, _ = _check(pl, phi, lab, g, 1, True)
    again = pl.group_sums(lab, g)
    assert np.array_equal(again[0].view(np.int64), sums.view(np.int64)) and np.array_equal(again[1].view(np.int64), diag.view(np.int64))


def test_one_group_is_the_total(synth_plan):
    pl, phi = synth_plan
    n = len(phi)
    sums, diag, rows, cols, form = pl.group_sums(np.zeros(n, dtype=np.int32), 1)
    total, total_diag, nr = pl.result_sums()
    assert form == 0 and rows.tolist() == [n] and cols.tolist() == [n] and nr == n
    assert abs(sums[0, 0] - total) <= GO.gamma(n * n) * total and abs(diag[0] - total_diag) <= GO.gamma(n) * total_diag
    assert sums[0, 0] == total and diag[0] == total_diag                 # (dyadic terms: both sums are exact)
    assert np.float32(pl.phi_mean_groups(np.zeros(n, dtype=np.int32))[0, 0]) == pl.phi_mean()


def test_row_shards_add_up(gen, synth_plan):
    pl_full, phi = synth_plan
    n = len(phi)
    rng = np.random.default_rng(7)
    for g, lab in ((64, _contiguous_labels(n, 64, rng)), (7, rng.integers(-1, 7, n).astype(np.int32))):
        full = pl_full.group_sums(lab, g)
        parts = []
        try:
            for rows in ((0, 1111), (1111, n)):
                pl_full.compute_device(device=0, rows=rows)
                shard = pl_full.result_to_host()
                assert shard.shape == (rows[1] - rows[0], n) and np.array_equal(shard, phi[rows[0]:rows[1]])
                parts.append(_check(pl_full, shard, lab, g, full[4], True, row_begin=rows[0]))
                with pytest.raises(ValueError):
                    pl_full.phi_mean_groups(lab, g)                       # needs all rows resident
        finally:
            pl_full.compute_device(device=0)                              # (the module's plan holds the full result again)
        ref = GO.group_sums(phi, lab, g)
        GO.assert_within_rule(parts[0][0] + parts[1][0], parts[0][1] + parts[1][1], ref)
        assert np.array_equal(parts[0][0] + parts[1][0], full[0]) and np.array_equal(parts[0][1] + parts[1][1], full[1])     # (exact terms)
        assert np.array_equal(parts[0][2] + parts[1][2], full[2]) and np.array_equal(parts[0][3], full[3]) and np.array_equal(parts[1][3], full[3])


# ---- errors -----------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_plan_usable(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(4000, 400, 10, skip_permille=50)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    n = len(pro)
    lab = (np.arange(n) * 5 // n).astype(np.int32)
    L, i32p = gen._capi.lib(), ctypes.POINTER(ctypes.c_int32)

    def good(phi):
        _check(pl, phi, lab, 5, 0, True)

    def c_call(labels, g):
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        return L.genphi_result_group_sums(pl._h, g, labels.ctypes.data_as(i32p), None, None, None, None, None)

    try:
        with pytest.raises(gen.GenphiDeviceError):                        # no resident result yet
            pl.group_sums(lab, 5)
        assert c_call(lab, 5) == gen._capi.GENPHI_ERR_DEVICE
        phi = pl.compute(device=0)
        good(phi)
        for bad in (5, -2):                                               # a label out of range
            wrong = lab.copy()
            wrong[n // 2] = bad
            with pytest.raises(ValueError):
                pl.group_sums(wrong, 5)
            assert c_call(wrong, 5) == gen._capi.GENPHI_ERR_ARG
            good(phi)
        for g in (0, CAP + 1):
            with pytest.raises(ValueError):
                pl.group_sums(np.zeros(n, dtype=np.int32), g)
            assert c_call(np.zeros(n, dtype=np.int32), g) == gen._capi.GENPHI_ERR_ARG
            good(phi)
        assert c_call(lab, 5) == 0                                        # every output pointer may be NULL
        pl.compute_device(device=0, storage64=True)                       # a Float64 result
        with pytest.raises(ValueError, match="Float32"):
            pl.group_sums(lab, 5)
        assert c_call(lab, 5) == gen._capi.GENPHI_ERR_ARG
        pl.compute_device(device=0)
        good(phi)
        pl.release_device()
        with pytest.raises(gen.GenphiDeviceError):
            pl.group_sums(lab, 5)
        pl.compute_device(device=0)
        good(phi)
        assert np.array_equal(pl.result_to_host(), phi)
    finally:
        pl.close()
