"""gen.phiEigen on host matrices and the numpy oracle of the device iteration (tests/phi_eigen_oracle.py), without a GPU: on the
committed genea140 oracle matrix both must agree with numpy.linalg.eigh.  Bounds, with u = 2^-53, lam_1 the largest eigenvalue and m
the steps taken:
  |theta_i - lam_i| <= residual_i + (N + 2) u lam_1   (some eigenvalue lies within the residual of a unit vector; the products that
                                                       measure the residual carry the second term; the top k + 1 eigenvalues are
                                                       asserted to lie further apart than that, so it is the one of rank i)
  residual_i        <= tol lam_1 + 8 (N + m + 2) u lam_1 for a converged pair (the Lanczos estimate is exact in exact arithmetic;
                                                       the product, two reorthogonalisation passes and the m-term Ritz sum round)"""
import os

import numpy as np
import pytest

import phi_eigen_oracle as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN140 = os.path.join(ROOT, "tests", "golden", "genea140_phi_oracle.npy")
U = 2.0 ** -53


@pytest.fixture(scope="module")
def golden():
    m = np.load(GOLDEN140)
    assert m.shape == (140, 140) and m.dtype == np.float32
    return m


def test_the_start_stream_is_splitmix64():
    """The first outputs of splitmix64 on seed 0 are published test vectors; the stream is a pure function of (seed, position)."""
    first = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    want = [2.0 * ((z >> 11) * 2.0 ** -53) - 1.0 for z in first]
    assert E.draws(0, 0, 3).tolist() == want
    assert np.array_equal(E.draws(7, 5, 10), E.draws(7, 0, 15)[5:])
    assert np.all(np.abs(E.draws(2 ** 64 - 1, 0, 1000)) <= 1.0)


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("k", [1, 4, 10])
def test_numpy_form_on_genea140(gen, golden, k, center):
    a = golden.astype(np.float64)
    b = E.centred(a) if center else a
    lam = np.linalg.eigvalsh(b)[::-1]
    got = gen.phiEigen(golden, k=k, center=center)
    assert got.values.shape == (k,) and got.vectors.shape == (140, k) and got.products == 0 and got.pro is None and got.center is center
    assert np.all(np.diff(got.values) <= 0)
    assert np.all(np.abs(got.values - lam[:k]) <= got.residual + 142 * U * lam[0])
    assert np.all(got.converged) and np.all(got.residual <= 1e-8 * lam[0])
    assert np.all(np.abs(np.linalg.norm(got.vectors, axis=0) - 1.0) <= 140 * U)
    big = np.argmax(np.abs(got.vectors), axis=0)
    assert np.all(got.vectors[big, np.arange(k)] > 0)                                   # the sign rule
    assert np.array_equal(got.coordinates, got.vectors * np.sqrt(np.maximum(got.values, 0.0)))
    if center:
        assert np.all(np.abs(got.vectors.sum(axis=0)) <= 1e-12)
    assert "PhiEigen: %d largest eigenpair" % k in repr(got)
    ids = np.arange(140) + 1000
    assert np.array_equal(gen.phiEigen(golden, k=k, center=center, probandIDs=ids).pro, ids)


def test_numpy_form_errors(gen, golden):
    for kw in (dict(k=0), dict(k=65), dict(k=141), dict(tol=-1.0), dict(tol=float("nan")), dict(k=5, maxiter=4), dict(maxiter=4097)):
        with pytest.raises(ValueError):
            gen.phiEigen(golden, **kw)
    with pytest.raises(ValueError):
        gen.phiEigen(golden[:3, :3], k=4)
    with pytest.raises(ValueError):
        gen.phiEigen(golden[:, :5])
    with pytest.raises(ValueError):
        gen.phiEigen(golden, probandIDs=[1, 2])
    one = gen.phiEigen(np.array([[0.5]], dtype=np.float32), k=1)
    assert one.values.tolist() == [0.5] and one.vectors.tolist() == [[1.0]]


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("k", [1, 4, 10])
def test_oracle_against_eigh_on_genea140(golden, k, center):
    a = golden.astype(np.float64)
    b = E.centred(a) if center else a
    lam, vec = np.linalg.eigh(b)
    lam, vec = lam[::-1], vec[:, ::-1]
    tol = 1e-8
    assert np.all(-np.diff(lam[:k + 1]) > 2 * tol * lam[0])                              # the near-double pair included
    got = E.lanczos(a, k, center=center, tol=tol, seed=0)
    m = got["products"]
    assert got["steps"][4 * tol] <= got["steps"][tol] == m <= got["steps"][tol / 4] <= 80
    assert np.all(got["converged"])
    assert np.all(np.abs(got["values"] - lam[:k]) <= got["residual"] + 142 * U * lam[0])
    assert np.all(got["residual"] <= tol * lam[0] + 8 * (140 + m + 2) * U * lam[0])
    gap = np.minimum(np.abs(np.diff(lam[:k + 1])), np.r_[np.inf, np.abs(np.diff(lam[:k]))])
    sine = np.sqrt(np.maximum(0.0, 1.0 - np.einsum("ij,ij->j", got["vectors"], vec[:, :k]) ** 2))
    assert np.all(sine <= got["residual"] / gap + 1e-7)                                  # Davis-Kahan (1 - cos^2 loses half the digits)


def test_oracle_on_half_the_identity_breaks_down_at_every_step():
    got = E.lanczos(np.eye(9) / 2, 4, tol=1e-8)
    assert got["products"] == 4 and got["values"].tolist() == [0.5] * 4 and np.all(got["converged"])
    assert np.abs(got["vectors"].T @ got["vectors"] - np.eye(4)).max() <= 16 * U
