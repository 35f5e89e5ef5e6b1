"""Host side of gen.phiCI / gen.fCI (no GPU): genphi_bootstrap_counts against the draws of tests/phi_ci_oracle.py, the host-matrix form
of gen.phiCI and gen.fCI against the statistic computed literally, the quantiles, the argument checks, and the errors that
genphi_result_bootstrap reports on a plan that has never computed."""
import ctypes
import math
import os

import numpy as np
import pytest

import phi_ci_oracle as CO
from simu_oracle import philox_scalar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN140 = os.path.join(ROOT, "tests", "golden", "genea140_phi_oracle.npy")
# geneaJi's kinship matrix (probands 1, 2, 29): every entry is a multiple of 2^-10
PHI_JI = np.array([[0.591796875, 0.37109375, 0.072265625], [0.37109375, 0.591796875, 0.072265625],
                   [0.072265625, 0.072265625, 0.53515625]], dtype=np.float32)
SEEDS = [0, 1, 0x1F2E3D4C5B6A7988]


def test_the_known_answers_of_the_header():
    for (n, seed, r, k), s in CO.KNOWN_DRAWS:
        o = philox_scalar((k >> 1, r, 0, 2), (seed & 0xFFFFFFFF, seed >> 32))           # (the scalar Philox: a third route)
        w = (o[0] | o[1] << 32) if k % 2 == 0 else (o[2] | o[3] << 32)
        assert (w * n) >> 64 == s == int(CO.draws(n, seed, r)[k])
        header = open(os.path.join(ROOT, "include", "genphi.h")).read()
        assert "%d, %s, %d, %d -> %d" % (n, hex(seed) if seed else "0", r, k, s) in header


@pytest.mark.parametrize("n, n_boot", [(2, 6), (3, 6), (140, 4), (65_537, 2)])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("first", [0, 37])
def test_counts_equal_the_oracle(gen, n, n_boot, seed, first):
    got = gen._capi.bootstrap_counts(n, seed, n_boot, first)
    assert got.dtype == np.int32 and got.shape == (n_boot, n)
    assert np.array_equal(got, CO.counts(n, seed, first, n_boot))
    assert np.all(got.sum(axis=1) == n) and got.min() >= 0


def test_counts_of_the_known_answers(gen):
    for (n, seed, r, k), s in CO.KNOWN_DRAWS:
        row = gen._capi.bootstrap_counts(n, seed, 1, r)[0]
        assert np.array_equal(row, np.bincount(CO.draws(n, seed, r), minlength=n)) and row[s] >= 1


def test_a_later_first_is_a_slice_and_large_calls_split_over_threads(gen):
    for seed in SEEDS:
        whole = gen._capi.bootstrap_counts(140, seed, 64)
        assert np.array_equal(gen._capi.bootstrap_counts(140, seed, 20, first=37), whole[37:57])
    big = gen._capi.bootstrap_counts(3000, 5, 1500)                           # (enough work for the threaded path)
    assert np.all(big.sum(axis=1) == 3000)
    assert np.array_equal(big[[0, 777, 1499]], np.stack([gen._capi.bootstrap_counts(3000, 5, 1, first=r)[0] for r in (0, 777, 1499)]))
    assert np.array_equal(big[1234], CO.counts(3000, 5, 1234, 1)[0])


def test_counts_argument_checks(gen):
    L, C = gen._capi.lib(), gen._capi
    buf = np.zeros(16, dtype=np.int32)
    p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    for n, first, n_boot, ptr in ((1, 0, 1, p), (0, 0, 1, p), (2 ** 31, 0, 1, p), (4, -1, 1, p), (4, 0, 0, p), (4, 2 ** 31 - 1, 1, p), (4, 0, 1, None)):
        assert L.genphi_bootstrap_counts(n, 0, first, n_boot, ptr) == C.GENPHI_ERR_ARG, (n, first, n_boot)
    assert L.genphi_bootstrap_counts(4, 0, 0, 4, p) == 0 and buf.sum() == 16
    for bad in (dict(n=1, seed=0, b=1), dict(n=4, seed=0, b=0), dict(n=4, seed=0, b=1, first=-1)):
        with pytest.raises(ValueError):
            gen._capi.bootstrap_counts(**bad)
    assert "genphi_bootstrap_counts" in C.EXPORTED_SYMBOLS and "genphi_result_bootstrap" in C.EXPORTED_SYMBOLS


def test_phiCI_of_the_geneaJi_matrix_equals_the_literal_oracle(gen):
    b = 40
    for seed in SEEDS:
        cnt = CO.counts(3, seed, 0, b)
        assert CO.exact_precondition(PHI_JI, cnt)                               # so every sum is exact: == whatever the order
        _, _, theta = CO.bootstrap(PHI_JI, seed, 0, b)
        got = gen.phiCI(PHI_JI, b=b, seed=seed)
        assert got.thetastar.dtype == np.float64 and np.array_equal(got.thetastar, theta)
        assert got.b == b and got.seed == seed and got.mean == gen.phiMean(PHI_JI) == np.float32(0.171875)
        assert np.array_equal(got.quantiles, np.quantile(theta, [0.025, 0.05, 0.95, 0.975])) and list(got.prob) == [0.025, 0.05, 0.95, 0.975]
    assert "PhiCI" in repr(got)


def test_phiCI_of_the_genea140_matrix_is_within_the_derived_bound(gen):
    phi = np.load(GOLDEN140)
    n, b, seed = 140, 12, SEEDS[2]
    quad, own, theta = CO.bootstrap(phi, seed, 0, b)
    got = gen.phiCI(phi, prob=[0.0, 0.5, 1.0], b=b, seed=seed)
    # theta = (quad - self) / (N (N - 1)) with quad within 3 N N 2^-53 and self within N 2^-53 relative of their exact sums
    bound = (3 * n * n * quad + n * own) * 2.0 ** -53 / (n * (n - 1)) + 4 * 2.0 ** -53 * theta
    print("largest error %.3e of the bound %.3e" % (np.max(np.abs(got.thetastar - theta)), np.min(bound)))
    assert np.all(np.abs(got.thetastar - theta) <= bound)
    assert np.array_equal(got.quantiles, np.quantile(got.thetastar, [0.0, 0.5, 1.0]))
    assert got.quantiles[0] == got.thetastar.min() and got.quantiles[2] == got.thetastar.max()
    assert got.mean == gen.phiMean(phi) and got.mean.dtype == np.float32
    again = gen.phiCI(phi, prob=0.5, b=b, seed=seed)                            # a scalar prob; the same seed, the same resamples
    assert np.array_equal(again.thetastar, got.thetastar) and again.quantiles.shape == (1,) and again.quantiles[0] == got.quantiles[1]
    assert np.array_equal(gen.phiCI(phi, b=5, seed=seed).thetastar, got.thetastar[:5])      # ... which do not depend on b
    fresh = gen.phiCI(phi, b=3)                                                # seed=None: fresh bits, reported
    assert 0 <= fresh.seed < 2 ** 64 and np.array_equal(gen.phiCI(phi, b=3, seed=fresh.seed).thetastar, fresh.thetastar)


def test_fCI_is_the_literal_mean_of_the_drawn_values(gen):
    rng = np.random.default_rng(7)
    for n in (2, 3, 140):
        F = rng.integers(0, 2 ** 12, n).astype(np.float64) / 2 ** 14            # inbreeding coefficients as gen.f gives them: dyadic
        b, seed = 30, SEEDS[1]
        got = gen.fCI(F, b=b, seed=seed)
        ref = np.array([math.fsum(F[CO.draws(n, seed, r)].tolist()) / n for r in range(b)])
        assert np.all(np.abs(got.thetastar - ref) <= n * 2.0 ** -53 * ref)
        assert np.array_equal(got.quantiles, np.quantile(got.thetastar, [0.025, 0.05, 0.95, 0.975]))
        assert got.mean == F.sum() / n and got.b == b and got.seed == seed


def test_value_errors(gen):
    phi = np.load(GOLDEN140)
    for kw in (dict(b=0), dict(b=-3), dict(prob=[0.5, 1.5]), dict(prob=-0.1), dict(prob=[math.nan])):
        with pytest.raises(ValueError):
            gen.phiCI(phi, seed=1, **kw)
        with pytest.raises(ValueError):
            gen.fCI(np.diagonal(phi) - 0.5, seed=1, **kw)
    for bad in (phi[:1, :1], phi[:3, :4], phi[0], np.zeros((0, 0), np.float32)):
        with pytest.raises(ValueError):
            gen.phiCI(bad, b=5, seed=1)
    for bad in ([0.25], [], phi[:2, :2]):
        with pytest.raises(ValueError):
            gen.fCI(bad, b=5, seed=1)
    ped = gen.genealogy(gen.geneaJi)
    with pytest.raises(KeyError):                                              # (before anything touches a device)
        gen.phiCI(ped, b=5, seed=1, probandIDs=[1, 2, 987654])
    with pytest.raises(ValueError):
        gen.phiCI(ped, b=5, seed=1, probandIDs=[29, 29])                        # duplicates collapse: one proband


def test_result_bootstrap_errors_without_a_device(gen):
    """The checks genphi_result_bootstrap makes before it looks for a device."""
    L, C = gen._capi.lib(), gen._capi
    ped = gen.genealogy(gen.geneaJi)
    dp = ctypes.POINTER(ctypes.c_double)
    q, s = np.zeros(4), np.zeros(4)

    def call(h, first, n_boot):
        return L.genphi_result_bootstrap(h, 1, first, n_boot, q.ctypes.data_as(dp), s.ctypes.data_as(dp), None)

    assert call(None, 0, 4) == C.GENPHI_ERR_ARG
    pl = gen.plan(ped)
    one = gen.plan(ped, [29])
    try:
        assert call(pl._h, 0, 0) == C.GENPHI_ERR_ARG and call(pl._h, -1, 4) == C.GENPHI_ERR_ARG
        assert call(pl._h, 2 ** 31 - 2, 4) == C.GENPHI_ERR_ARG
        assert call(one._h, 0, 4) == C.GENPHI_ERR_ARG and "2 probands" in C.last_error()
        assert call(pl._h, 0, 4) == C.GENPHI_ERR_DEVICE                          # nothing resident
        with pytest.raises(gen.GenphiDeviceError):
            pl.bootstrap(4, 1)
        with pytest.raises(ValueError):
            pl.bootstrap(0, 1)
        with pytest.raises(ValueError):
            one.bootstrap(4, 1)
    finally:
        pl.close()
        one.close()
