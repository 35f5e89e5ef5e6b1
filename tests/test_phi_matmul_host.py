"""gen.phiMatmul / gen.phiSolve on host matrices, without a GPU: the numpy Float64 forms of the definitions in include/genphi.h, on the
committed genea140 oracle matrix and on small symmetric positive definite matrices with known answers.  The solve is held to the same
derived bounds as on the device (tests/test_phi_solve_gpu.py): with A = Phi + ridge I, lam its extreme eigenvalues, u = 2^-53,
  rounding = 2 (N + 2) u || |A| |z| + |b| || / ||b||;  |residual - recomputed| <= rounding;
  ||z - z*|| <= (||r|| + ||r*|| + rounding ||b||) / lam_min;  iterations <= the classical CG bound + 1."""
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN140 = os.path.join(ROOT, "tests", "golden", "genea140_phi_oracle.npy")
U = 2.0 ** -53
TOL = 1e-10


@pytest.fixture(scope="module")
def golden():
    m = np.load(GOLDEN140)
    assert m.shape == (140, 140) and m.dtype == np.float32
    return m


def iteration_bound(lam, tol):
    s = math.sqrt(lam[-1] / lam[0])
    if s <= 1.0:
        return 2
    return math.ceil(math.log(tol / (2.0 * s)) / math.log((s - 1.0) / (s + 1.0))) + 1


def check(phi, b, got, ridge, tol=TOL, converged=True):
    n = len(phi)
    b2 = b[:, None] if b.ndim == 1 else b
    z = got.solution[:, None] if b.ndim == 1 else got.solution
    A = phi.astype(np.float64) + ridge * np.eye(n)
    lam = np.linalg.eigvalsh(A)
    assert got.solution.shape == b.shape and got.solution.dtype == np.float64
    assert got.residual.shape == got.iterations.shape == got.converged.shape == (b2.shape[1],)
    assert got.iterations.dtype == np.int32 and got.converged.dtype == bool and np.array_equal(got.converged, got.residual <= tol)
    zstar = np.linalg.solve(A, b2)
    for c in range(b2.shape[1]):
        nb = np.linalg.norm(b2[:, c])
        if nb == 0:
            assert got.iterations[c] == 0 and got.residual[c] == 0 and not z[:, c].any() and got.converged[c]
            continue
        r, rstar = b2[:, c] - A @ z[:, c], b2[:, c] - A @ zstar[:, c]
        rounding = 2 * (n + 2) * U * np.linalg.norm(np.abs(A) @ np.abs(z[:, c]) + np.abs(b2[:, c])) / nb
        assert abs(got.residual[c] - np.linalg.norm(r) / nb) <= rounding
        assert np.linalg.norm(z[:, c] - zstar[:, c]) <= (np.linalg.norm(r) + np.linalg.norm(rstar) + rounding * nb) / lam[0]
        if converged:
            assert got.converged[c] and 1 <= got.iterations[c] <= iteration_bound(lam, tol)


def rhs(n, seed):
    b = np.random.default_rng(seed).standard_normal((n, 8))
    b[:, 6] = 1.0
    b[:, 7] = 0.0
    return b


# ---- phiMatmul --------------------------------------------------------------------------------------------------------------------

def test_matmul_shapes_and_values(gen, golden):
    X = np.random.default_rng(1).integers(-1000, 1001, size=(140, 70)).astype(np.float64)      # exact: see tests/test_phi_matmul_gpu.py
    ref = golden.astype(np.float64) @ X
    got = gen.phiMatmul(golden, X)
    assert got.shape == (140, 70) and got.dtype == np.float64 and np.array_equal(got, ref)
    one = gen.phiMatmul(golden, X[:, 3])
    assert one.shape == (140,) and np.array_equal(one, ref[:, 3])
    assert np.array_equal(gen.phiMatmul(golden, X[:, 3:4]), ref[:, 3:4])
    assert np.array_equal(gen.phiMatmul(golden, np.eye(140)), golden.astype(np.float64))
    assert np.array_equal(gen.phiMatmul(golden.astype(np.float64), list(range(140))), ref[:, 0] * 0 + golden.astype(np.float64) @ np.arange(140.0))
    assert np.array_equal(gen.phiMatmul([[0.5, 0.25], [0.25, 0.5]], [1, 2]), [1.0, 1.25])
    assert gen.phiMatmul(golden, np.zeros((140, 0))).shape == (140, 0)


def test_matmul_argument_errors(gen, golden):
    for bad in (np.ones(139), np.ones((141, 2)), np.ones((2, 140)), np.ones((140, 2, 2))):
        with pytest.raises(ValueError):
            gen.phiMatmul(golden, bad)
    for m in (np.ones((3, 4)), np.ones(5), np.ones((2, 2, 2))):
        with pytest.raises(ValueError, match="square"):
            gen.phiMatmul(m, np.ones(3))
    with pytest.raises(ValueError, match="probandIDs"):
        gen.phiMatmul(golden, np.ones(140), probandIDs=[1, 2, 3])


# ---- phiSolve ---------------------------------------------------------------------------------------------------------------------

def test_known_answers(gen):
    got = gen.phiSolve(np.eye(4) / 2, [1.0, -2.0, 4.0, 0.5])                                   # one step: every direction is an eigenvector
    assert got.solution.tolist() == [2.0, -4.0, 8.0, 1.0] and got.iterations.tolist() == [1] and got.residual.tolist() == [0.0]
    got = gen.phiSolve(np.eye(4) / 2, [1.0, -2.0, 4.0, 0.5], ridge=1.5)
    assert got.solution.tolist() == [0.5, -1.0, 2.0, 0.25] and got.converged.tolist() == [True] and got.ridge == 1.5
    m = np.array([[0.5, 0.25], [0.25, 0.5]])                                                   # eigenvalues 0.75 and 0.25: two steps
    got = gen.phiSolve(m, np.array([[1.0, 1.0, 0.0], [1.0, -1.0, 0.0]]))
    assert got.iterations.tolist() == [1, 1, 0] and np.array_equal(got.solution, [[4.0 / 3.0, 4.0, 0.0], [4.0 / 3.0, -4.0, 0.0]])
    got = gen.phiSolve(m, [1.0, 0.0])
    assert got.iterations.tolist() == [2] and np.allclose(got.solution, np.linalg.solve(m, [1.0, 0.0]), rtol=0, atol=1e-15)
    check(m.astype(np.float32), np.array([1.0, 0.0]), got, 0.0)


@pytest.mark.parametrize("ridge", [0.0, 0.5])
def test_genea140(gen, golden, ridge):
    b = rhs(140, 140)
    got = gen.phiSolve(golden, b, ridge=ridge)
    check(golden, b, got, ridge)
    assert got.pro is None and len(got) == 140 and got.tol == TOL
    again = gen.phiSolve(golden, b, ridge=ridge)
    assert again.solution.tobytes() == got.solution.tobytes() and again.residual.tobytes() == got.residual.tobytes()
    one = gen.phiSolve(golden, b[:, 6], ridge=ridge, probandIDs=np.arange(1000, 1140))
    assert one.solution.shape == (140,) and one.solution.tobytes() == np.ascontiguousarray(got.solution[:, 6]).tobytes()
    assert one.iterations[0] == got.iterations[6] and np.array_equal(one.pro, np.arange(1000, 1140))
    if ridge == 0.0:
        assert got.iterations[:7].max() <= 13                                                  # the bound for this matrix: 12 + 1
    text = repr(got)
    assert text.startswith("PhiSolve: (Phi + %g I) z = b for 140 probands, 8 right-hand sides; 8 converged" % ridge) and "iterations 0 .. " in text


def test_maxiter_and_breakdown(gen, golden):
    b = rhs(140, 7)
    got = gen.phiSolve(golden, b, maxiter=2)
    assert got.iterations.tolist() == [2] * 7 + [0] and np.all(got.residual[:7] > TOL) and got.converged.tolist() == [False] * 7 + [True]
    check(golden, b, got, 0.0, converged=False)
    neg = gen.phiSolve(-np.eye(3), [1.0, 2.0, 3.0])                                            # negative curvature: the column stops at once
    assert neg.iterations.tolist() == [1] and not neg.solution.any() and neg.residual.tolist() == [1.0] and not neg.converged[0]
    nan = gen.phiSolve(np.eye(3), [1.0, np.nan, 3.0])
    assert nan.iterations.tolist() == [1] and not nan.solution.any() and np.isnan(nan.residual[0]) and not nan.converged[0]


def test_solve_argument_errors(gen, golden):
    b = np.ones(140)
    for kw in (dict(ridge=-1.0), dict(ridge=math.inf), dict(ridge=math.nan), dict(tol=-1e-3), dict(tol=math.nan), dict(maxiter=0), dict(maxiter=-1)):
        with pytest.raises(ValueError):
            gen.phiSolve(golden, b, **kw)
    for bad in (np.ones(139), np.ones((141, 2)), np.ones((140, 2, 2))):
        with pytest.raises(ValueError):
            gen.phiSolve(golden, bad)
    with pytest.raises(ValueError, match="square"):
        gen.phiSolve(np.ones((3, 4)), np.ones(3))
    with pytest.raises(ValueError, match="probandIDs"):
        gen.phiSolve(golden, b, probandIDs=[1, 2])
    assert gen.phiSolve(golden, b, tol=0.0, maxiter=3).iterations.tolist() == [3]              # tol = 0 is allowed: it runs to maxiter
