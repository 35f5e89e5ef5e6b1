"""genphi_result_solve / PhiPlan.solve / gen.phiSolve on the GPU (include/genphi.h): conjugate gradients over the device
product.  Every bound below is derived, none is measured.  With A = Phi + ridge I from the host copy in Float64, its extreme
eigenvalues lam from numpy.linalg.eigvalsh, u = 2^-53:
  rounding(z, b) = 2 (N + 2) u || |A| |z| + |b| || / ||b||     what two Float64 products of length N can differ by, relative to ||b||
  |reported residual - recomputed residual| <= rounding
  ||z - z*|| <= (||r|| + ||r*|| + rounding ||b||) / lam_min       from z - z* = A^-1 (r* - r); z* = numpy.linalg.solve(A, b)
  iterations <= ceil(ln(tol / (2 sqrt(kappa))) / ln((sqrt(kappa) - 1) / (sqrt(kappa) + 1))) + 1    the classical CG bound carried to the
                                                                                                 residual norm, kappa = lam_max / lam_min"""
import ctypes
import math
import os

import numpy as np
import pytest

from test_phi_over_gpu import synth_case                    # noqa: F401  (the 2,500 probands of the phiOver tests: a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN140 = os.path.join(ROOT, "tests", "golden", "genea140_phi_oracle.npy")
U = 2.0 ** -53
TOL = 1e-10
DP = ctypes.POINTER(ctypes.c_double)


def rhs(n, seed):
    """Eight right-hand sides: six standard normal columns, a ones column, a zero column."""
    b = np.random.default_rng(seed).standard_normal((n, 8))
    b[:, 6] = 1.0
    b[:, 7] = 0.0
    return b


def iteration_bound(lam, tol):
    kappa = lam[-1] / lam[0]
    s = math.sqrt(kappa)
    if s <= 1.0:
        return 2
    return math.ceil(math.log(tol / (2.0 * s)) / math.log((s - 1.0) / (s + 1.0))) + 1


def check_solution(phi, b, ridge, tol, z, residual, iterations, expect_converged=True):
    n = len(phi)
    A = phi.astype(np.float64) + ridge * np.eye(n)
    lam = np.linalg.eigvalsh(A)
    assert lam[0] > 0
    zero = ~b.any(axis=0)
    assert z.shape == b.shape and residual.shape == iterations.shape == (b.shape[1],) and iterations.dtype == np.int32
    assert np.all(iterations[zero] == 0) and not z[:, zero].any() and np.all(residual[zero] == 0)
    cap = iteration_bound(lam, tol)
    print("ridge %g: eigenvalues %.4g .. %.4g, iterations %s (bound %d), residuals %s" % (ridge, lam[0], lam[-1], iterations.tolist(), cap, residual.tolist()))
    if expect_converged:
        assert np.all(residual <= tol)
        assert np.all(iterations[~zero] >= 1) and np.all(iterations <= cap)
    zstar = np.linalg.solve(A, b)
    for c in np.nonzero(~zero)[0]:
        nb = np.linalg.norm(b[:, c])
        r, rstar = b[:, c] - A @ z[:, c], b[:, c] - A @ zstar[:, c]
        rounding = 2 * (n + 2) * U * np.linalg.norm(np.abs(A) @ np.abs(z[:, c]) + np.abs(b[:, c])) / nb
        assert abs(residual[c] - np.linalg.norm(r) / nb) <= rounding, c
        assert np.linalg.norm(z[:, c] - zstar[:, c]) <= (np.linalg.norm(r) + np.linalg.norm(rstar) + rounding * nb) / lam[0], c


def run(pl, phi, ridge, seed):
    b = rhs(len(phi), seed)
    z, res, its = pl.solve(b, ridge=ridge, tol=TOL)
    check_solution(phi, b, ridge, TOL, z, res, its)
    again = pl.solve(b, ridge=ridge, tol=TOL)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((z, res, its), again))
    one = pl.solve(b[:, 2], ridge=ridge, tol=TOL)                            # a 1-D B; the column's own scalars: the same bytes alone
    assert one[0].shape == (len(phi),) and one[0].tobytes() == np.ascontiguousarray(z[:, 2]).tobytes()
    assert one[1][0] == res[2] and one[2][0] == its[2]
    return b, z, res, its


@pytest.mark.parametrize("ridge", [0.0, 0.5])
def test_geneaJi(gen, ridge):
    pl = gen.plan(gen.genealogy(gen.geneaJi))
    try:
        phi = pl.compute(device=0)
        run(pl, phi, ridge, 3)
    finally:
        pl.close()


@pytest.mark.parametrize("ridge", [0.0, 0.5])
def test_genea140(gen, ridge):
    golden = np.load(GOLDEN140)
    ped = gen.genealogy(gen.genea140)
    pl = gen.plan(ped)
    try:
        pl.compute_device(device=0)
        b, z, res, its = run(pl, golden, ridge, 140)
    finally:
        pl.close()
    got = gen.phiSolve(ped, b, ridge=ridge, device=0)
    assert got.solution.tobytes() == z.tobytes() and got.residual.tobytes() == res.tobytes() and got.iterations.tobytes() == its.tobytes()
    assert np.array_equal(got.pro, gen.pro(ped)) and np.all(got.converged) and got.converged.dtype == bool
    assert "8 right-hand sides; 8 converged" in repr(got)


@pytest.mark.parametrize("ridge", [0.0, 0.5])
def test_synthetic_case(synth_case, ridge):
    pl, phi = synth_case[2], synth_case[3]
    run(pl, phi, ridge, 2500)


def test_maxiter_2_returns_what_it_has(synth_case):
    pl, phi = synth_case[2], synth_case[3]
    b = rhs(2500, 2500)
    z, res, its = pl.solve(b, tol=TOL, maxiter=2)
    assert its.tolist() == [2] * 7 + [0] and np.all(res[:7] > TOL) and res[7] == 0
    check_solution(phi, b, 0.0, TOL, z, res, its, expect_converged=False)


def test_more_than_64_right_hand_sides_run_as_blocks(synth_case):
    pl = synth_case[2]
    b = np.random.default_rng(70).standard_normal((2500, 70))
    z, res, its = pl.solve(b, ridge=1.0, tol=1e-6)
    assert z.shape == (2500, 70) and np.all(res <= 1e-6)
    z1, res1, its1 = pl.solve(b[:, 66], ridge=1.0, tol=1e-6)
    assert z1.tobytes() == np.ascontiguousarray(z[:, 66]).tobytes() and res1[0] == res[66] and its1[0] == its[66]


def test_phiSolve_of_a_pedigree_names_the_probands(gen, synth_case):
    ped, pro, pl, _, _ = synth_case
    b = rhs(2500, 1)[:, 5:]
    got = gen.phiSolve(ped, b, ridge=0.5, probandIDs=np.concatenate([pro[:3], pro]), device=0)       # duplicates collapse
    z, res, its = pl.solve(b, ridge=0.5)
    assert got.solution.tobytes() == z.tobytes() and got.residual.tobytes() == res.tobytes() and got.iterations.tobytes() == its.tobytes()
    assert np.array_equal(got.pro, pro) and got.converged.tolist() == [True, True, True] and got.ridge == 0.5 and got.tol == 1e-10


def test_errors_leave_the_plan_usable(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(4000, 400, 10, skip_permille=50)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    L, C = gen._capi.lib(), gen._capi
    b = rhs(400, 400)
    z, res, its = np.full((400, 8), -7.0), np.full(8, -7.0), np.full(8, -7, np.int32)
    pb, pz, pr, pi = b.ctypes.data_as(DP), z.ctypes.data_as(DP), res.ctypes.data_as(DP), its.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    def call(h=None, k=8, bb=pb, ldb=8, ridge=0.0, tol=TOL, max_iter=100, zz=pz, ldz=8):
        return L.genphi_result_solve(h if h is not None else pl._h, k, bb, ldb, ridge, tol, max_iter, zz, ldz, pr, pi)

    try:
        with pytest.raises(gen.GenphiDeviceError):                        # no resident result yet
            pl.solve(b)
        assert call() == C.GENPHI_ERR_DEVICE
        phi = pl.compute(device=0)
        sums = pl.result_sums()
        want = pl.solve(b)
        check_solution(phi, b, 0.0, TOL, *want)

        def good():
            assert all(x.tobytes() == y.tobytes() for x, y in zip(pl.solve(b), want))
            assert pl.result_sums() == sums and np.array_equal(pl.result_to_host(), phi)

        assert L.genphi_result_solve(None, 8, pb, 8, 0.0, TOL, 100, pz, 8, pr, pi) == C.GENPHI_ERR_ARG
        for kw in (dict(k=0), dict(k=65), dict(bb=None), dict(zz=None), dict(ldb=7), dict(ldz=7), dict(ridge=-1.0), dict(ridge=math.inf), dict(ridge=math.nan),
                   dict(tol=-1e-3), dict(tol=math.nan), dict(max_iter=0), dict(max_iter=-5)):
            assert call(**kw) == C.GENPHI_ERR_ARG, kw
            assert "genphi_result_solve" in C.last_error()
        good()
        for kw in (dict(ridge=-1.0), dict(ridge=math.inf), dict(tol=-1.0), dict(tol=math.nan), dict(maxiter=0)):
            with pytest.raises(ValueError):
                pl.solve(b, **kw)
        with pytest.raises(ValueError):
            pl.solve(np.ones(399))
        pl.compute_device(device=0, rows=(100, 300))                      # a shard cannot solve
        with pytest.raises(ValueError, match="shard"):
            pl.solve(b)
        assert call() == C.GENPHI_ERR_ARG
        pl.compute_device(device=0, rows=(7, 7))                          # nor can an empty one
        assert call() == C.GENPHI_ERR_ARG
        pl.compute_device(device=0, storage64=True)                       # a Float64 result
        with pytest.raises(ValueError, match="Float32"):
            pl.solve(b)
        assert call() == C.GENPHI_ERR_ARG
        pl.compute_device(device=0)
        good()
        pl.release_device()
        with pytest.raises(gen.GenphiDeviceError):
            pl.solve(b)
        assert call() == C.GENPHI_ERR_DEVICE
        assert np.all(z == -7.0) and np.all(res == -7.0) and np.all(its == -7)      # no failed call wrote anything
        pl.compute_device(device=0)
        good()
        assert call() == 0 and z.tobytes() == want[0].tobytes() and res.tobytes() == want[1].tobytes() and its.tobytes() == want[2].tobytes()
    finally:
        pl.close()
