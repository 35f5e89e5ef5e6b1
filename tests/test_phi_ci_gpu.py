"""genphi_result_bootstrap / PhiPlan.bootstrap / gen.phiCI on the GPU against tests/phi_ci_oracle.py, on the host matrix of the same
plan.  Two kinds of check: `==` where every partial sum is exact in Float64 (asserted on the CPU first: phi_ci_oracle.exact_precondition),
and the derived bound elsewhere: all terms are >= 0 and every product c_j Phi_ij is exact, so quad is within 3 n_rows N 2^-53
relative of the exact sum and self within n_rows 2^-53 (include/genphi.h); a Float32 accumulation would miss it by four orders.

A workgroup of the product kernel (csrc/bootstrap.hip) owns 128 rows x 128 resamples and walks the columns in chunks of 16; the
row pitch is a multiple of 64.  The sizes below sit on those edges and one to either side."""
import ctypes

import numpy as np
import pytest

import phi_ci_oracle as CO
from random_pedigree import random_pedigree

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SEED = 0x9E3779B97F4A7C15
ROW_EDGES = [2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257, 1025]          # column chunk 16, pitch 64, row block 128, several blocks
B_EDGES = [1, 65, 127, 128, 129]                                            # resample tile 128 (and the issue's 1 and 65)


def _within_bound(got, ref, n_rows, n):
    quad, own = got
    rq, ro = ref
    eq, eo = np.abs(quad - rq), np.abs(own - ro)
    print("quad: largest error %.3e (bound %.3e x quad); self: %.3e (bound %.3e x self)"
          % (np.max(eq / np.maximum(rq, 1e-300)), 3 * n_rows * n * U, np.max(eo / np.maximum(ro, 1e-300)), n_rows * U))
    return bool(np.all(eq <= 3 * n_rows * n * U * rq) and np.all(eo <= n_rows * U * ro))


def _theta(quad, own, n):
    return (quad - own) / (float(n) * (n - 1))


# ---- geneaJi ------------------------------------------------------------------------------------------------------------------

def test_geneaJi(gen):
    ped = gen.genealogy(gen.geneaJi)
    pl = gen.plan(ped)
    try:
        phi = pl.compute(device=0)
        assert phi.shape == (3, 3) and CO.exact_precondition(phi, CO.counts(3, SEED, 0, 5))
        rq, ro, rt = CO.bootstrap(phi, SEED, 0, 5)
        quad, own = pl.bootstrap(5, SEED)
        assert quad.dtype == np.float64 and np.array_equal(quad, rq) and np.array_equal(own, ro)
        assert np.array_equal(_theta(quad, own, 3), rt)
    finally:
        pl.close()
    got = gen.phiCI(ped, b=5, seed=SEED, device=0)
    assert np.array_equal(got.thetastar, rt) and got.mean == np.float32(0.171875) and got.b == 5 and got.seed == SEED
    assert np.array_equal(got.quantiles, np.quantile(rt, [0.025, 0.05, 0.95, 0.975]))
    assert np.array_equal(gen.phiCI(ped, b=5, seed=SEED, probandIDs=[1, 2, 29, 2], device=0).thetastar, rt)     # duplicates collapse


# ---- genea140 -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def g140(gen):
    """(pedigree, host matrix, the oracle's (quad, self, theta) of 130 resamples)."""
    ped = gen.genealogy(gen.genea140)
    pl = gen.plan(ped)
    try:
        phi = pl.compute(device=0)
    finally:
        pl.close()
    assert phi.shape == (140, 140)
    return ped, phi, CO.bootstrap(phi, SEED, 0, 130)


@pytest.mark.parametrize("panel", [64, None, 1, 7])
def test_genea140_forced_and_default_panels(gen, g140, panel):
    """b = 130 with panels of 64: two full panels and a ragged one of 2."""
    ped, phi, (rq, ro, rt) = g140
    pl = gen.plan(ped, tuning={} if panel is None else {"BOOT_PANEL": panel})
    try:
        assert np.array_equal(pl.compute(device=0), phi)
        b = 130 if panel in (64, None) else 20
        quad, own = pl.bootstrap(b, SEED)
        assert _within_bound((quad, own), (rq[:b], ro[:b]), 140, 140)
        again = pl.bootstrap(b, SEED)
        assert again[0].tobytes() == quad.tobytes() and again[1].tobytes() == own.tobytes()
        assert np.all(np.abs(_theta(quad, own, 140) - rt[:b]) <= (3 * 140 * 140 * rq[:b] + 140 * ro[:b]) * U / (140 * 139) + 4 * U * rt[:b])
        part = pl.bootstrap(20, SEED, first=37)                                # the prefix property on the device
        whole = pl.bootstrap(64, SEED)
        assert part[0].tobytes() == whole[0][37:57].tobytes() and part[1].tobytes() == whole[1][37:57].tobytes()
        k = min(b, 64)
        assert whole[0][:k].tobytes() == quad[:k].tobytes() and whole[1][:k].tobytes() == own[:k].tobytes()
    finally:
        pl.close()


def test_phiCI_of_a_pedigree_and_of_its_matrix_agree(gen, g140):
    ped, phi, (rq, ro, rt) = g140
    dev = gen.phiCI(ped, b=200, seed=SEED, device=0)
    host = gen.phiCI(gen.phi(ped, device=0), b=200, seed=SEED)
    bound = (3 * 140 * 140 * rq.max() + 140 * ro.max()) * U / (140 * 139) * 4
    assert np.all(np.abs(dev.thetastar - host.thetastar) <= bound)
    assert np.all(np.abs(dev.thetastar[:130] - rt) <= bound)
    assert np.all(np.abs(dev.quantiles - host.quantiles) <= 1e-12 * host.quantiles)
    assert host.mean == gen.phiMean(phi) and dev.b == 200 and dev.seed == SEED
    # the pedigree form reduces the resident matrix in Float64 and rounds once (PhiPlan.phi_mean); gen.phiMean adds in Float32
    p64 = phi.astype(np.float64)
    exact = np.float32((p64.sum() - np.trace(p64)) / (140 * 139))
    assert dev.mean.dtype == np.float32 and abs(dev.mean - exact) <= np.spacing(exact)


# ---- shallow random pedigrees: exact inputs ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def shallow(gen):
    """4,000 individuals, at most 8 generations deep, the probands taken from the youngest: kinships are multiples of a small power
    of two, so that the sums of a resample are exact in Float64."""
    rng = np.random.default_rng(2024)
    ind, fa, mo, _ = random_pedigree(rng, 4000, p_founder=0.05, p_one_parent=0.1, p_selfing=0.02, max_back=400, max_depth=8)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=False)
    return ped, ind


def _exact_case(gen, shallow, n, b, tuning):
    """(plan with the full result resident, host matrix, oracle (quad, self, theta) of b resamples), the precondition asserted."""
    ped, ind = shallow
    pl = gen.plan(ped, ind[-n:], tuning=tuning)
    phi = pl.compute(device=0)
    assert phi.shape == (n, n) and pl.result_device()[1] % 64 == 0
    assert CO.exact_precondition(phi, CO.counts(n, SEED, 0, b))
    s = CO.draws(n, SEED, 0)
    assert CO.theta_literal(phi, s, exact=True) == CO.theta_literal(phi, s)      # numpy's sum is fsum's here
    return pl, phi, CO.bootstrap(phi, SEED, 0, b, exact=True)


@pytest.mark.parametrize("n", ROW_EDGES)
def test_exact_inputs_equal_the_oracle_at_every_tile_edge(gen, shallow, n):
    pl, phi, ref = _exact_case(gen, shallow, n, max(B_EDGES), {})
    try:
        for b in B_EDGES:
            quad, own = pl.bootstrap(b, SEED)
            assert np.array_equal(quad, ref[0][:b]) and np.array_equal(own, ref[1][:b]), b
            assert np.array_equal(_theta(quad, own, n), ref[2][:b])
    finally:
        pl.close()


def test_row_shards_add_up_and_the_panel_width_changes_no_bit(gen, shallow):
    n, b = 257, 65
    pl, phi, (rq, ro, _) = _exact_case(gen, shallow, n, b, {})
    try:
        full = pl.bootstrap(b, SEED)
        assert np.array_equal(full[0], rq) and np.array_equal(full[1], ro)
        total = [np.zeros(b), np.zeros(b)]
        for r0, r1 in ((0, 100), (100, 257), (257, 257)):
            pl.compute_device(device=0, rows=(r0, r1))
            quad, own = pl.bootstrap(b, SEED)
            sq, so, _ = CO.bootstrap(phi, SEED, 0, b, row_begin=r0, row_end=r1, exact=True)
            assert np.array_equal(quad, sq) and np.array_equal(own, so), (r0, r1)
            if r0 == r1:
                assert not quad.any() and not own.any()
            total[0] += quad
            total[1] += own
        assert np.array_equal(total[0], full[0]) and np.array_equal(total[1], full[1])
    finally:
        pl.close()
    for panel in (1, 7, 64):
        pl = gen.plan(shallow[0], shallow[1][-n:], tuning={"BOOT_PANEL": panel})
        try:
            pl.compute_device(device=0)
            quad, own = pl.bootstrap(b, SEED)
            assert quad.tobytes() == full[0].tobytes() and own.tobytes() == full[1].tobytes(), panel
        finally:
            pl.close()


# ---- errors -----------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_plan_usable(gen, g140):
    ped, phi, (rq, ro, _) = g140
    L, C = gen._capi.lib(), gen._capi
    dp = ctypes.POINTER(ctypes.c_double)
    q, s = np.full(4, -7.0), np.full(4, -7.0)
    pl = gen.plan(ped)
    one = gen.plan(ped, gen.pro(ped)[:1])

    def c_call(h, first, n_boot):
        return L.genphi_result_bootstrap(h, SEED, first, n_boot, q.ctypes.data_as(dp), s.ctypes.data_as(dp), None)

    def good():
        quad, own = pl.bootstrap(4, SEED)
        assert _within_bound((quad, own), (rq[:4], ro[:4]), 140, 140)
        assert np.array_equal(pl.result_to_host(), phi)

    try:
        assert c_call(pl._h, 0, 4) == C.GENPHI_ERR_DEVICE                        # no resident result yet
        with pytest.raises(gen.GenphiDeviceError):
            pl.bootstrap(4, SEED)
        pl.compute_device(device=0)
        good()
        assert c_call(pl._h, 0, 0) == C.GENPHI_ERR_ARG
        good()
        assert c_call(pl._h, -1, 4) == C.GENPHI_ERR_ARG
        good()
        assert np.all(q == -7.0) and np.all(s == -7.0)                          # no failed call wrote anything
        pl.compute_device(device=0, storage64=True)                             # a Float64 result
        assert c_call(pl._h, 0, 4) == C.GENPHI_ERR_ARG
        with pytest.raises(ValueError, match="Float32"):
            pl.bootstrap(4, SEED)
        pl.compute_device(device=0)
        good()
        one.compute_device(device=0)                                            # a one-proband plan
        assert c_call(one._h, 0, 4) == C.GENPHI_ERR_ARG
        with pytest.raises(ValueError):
            one.bootstrap(4, SEED)
        good()
        pl.release_device()
        assert c_call(pl._h, 0, 4) == C.GENPHI_ERR_DEVICE
        pl.compute_device(device=0)
        good()
        n_rows = ctypes.c_int64(-1)
        assert L.genphi_result_bootstrap(pl._h, SEED, 0, 4, None, None, ctypes.byref(n_rows)) == 0 and n_rows.value == 140
    finally:
        pl.close()
        one.close()
