"""genphi_result_eigen / PhiPlan.eigen / gen.phiEigen on the GPU (include/genphi.h), against numpy.linalg.eigh of the
host copy of the same matrix and against the numpy restatement of the iteration (tests/phi_eigen_oracle.py).

Every bound is derived, none is taken from what the device returns.  With u = 2^-53, N probands, m the products taken, lam the
eigenvalues by eigh (descending), theta / v / residual what the call returns, and theta_1 its largest value:

  rounding(N, m) = c (N + m + 2) u theta_1 with c = 3 sqrt(m) + 3.  One product rounds by (N + 2) u |Phi| |x|, in norm at most
      (N + 2) u lam_1 for a unit x (Phi >= 0 entrywise).  A Lanczos step is one product and two Gram-Schmidt passes of m terms each:
      its column of A V = V T + beta v e^T + F has |F_j| <= ((N + 2) + 2 (m + 2)) u lam_1 <= 3 (N + m + 2) u lam_1, and
      |F s| <= |s|_1 max_j |F_j| <= sqrt(m) max_j |F_j| for a unit s: the 3 sqrt(m).  The + 3: the product that measures the residual,
      the m-term fma chain of the Ritz vector, and the eigenvectors of T with the normalisations.
  |theta_i - lam_i| <= residual_i + rounding          (an eigenvalue lies within the residual of a unit vector; the top k + 1 eigenvalues
                                                       are first asserted to lie more than 2 tol lam_1 apart, so it is the i-th)
  theta_i <= lam_i + rounding                          (interlacing: Ritz values of a compression never exceed the eigenvalue of their rank)
  sin angle(v_i, eigh's vector) <= (residual_i + rounding) / gap_i, gap_i the distance from theta_i to the other eigenvalues
                                                       (Davis-Kahan, sin-theta theorem for one vector)
  residual_i <= tol theta_1 + rounding                 where the pair is flagged converged (the estimate beta |s| is the residual in exact
                                                       arithmetic)
  |V^T V - I|_max <= (m + 2) max(that of eigh's own k vectors, (N + 2) u): a Ritz vector is a sum of m basis vectors, each orthogonal
                                                       to the others to a few u after two passes; both figures are printed
  products within [oracle's step for 4 tol, oracle's step for tol / 4]: rounding moves the estimate by far less than a factor 4, a lost
                                                       reorthogonalisation shows as extra steps and ghost copies."""
import ctypes
import os

import numpy as np
import pytest

import phi_eigen_oracle as E
from test_phi_over_gpu import synth_case                    # noqa: F401  (the 2,500 probands of the phiOver tests: a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN140 = os.path.join(ROOT, "tests", "golden", "genea140_phi_oracle.npy")
U = 2.0 ** -53
TOL = 1e-8
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int32)
# by the kernels' names: csrc/eigen.hip kEigStep (entries a workgroup takes per step of a sum); csrc/matmul.hip kMmStep, kMmChunkNarrow
# (columns of a step and of a staged chunk of the one-column product; its row block of 32 divides them)
EIG_STEP, MM_STEP, MM_CHUNK = 512, 256, 1024
SIZES = [1, 2, 5, MM_STEP - 1, MM_STEP, MM_STEP + 1, EIG_STEP - 1, EIG_STEP + 1, MM_CHUNK - 1, MM_CHUNK + 1]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def rounding(n, m, top):
    return (3.0 * np.sqrt(m) + 3.0) * (n + m + 2) * U * top


def spectrum(phi, center):
    a = np.asarray(phi, dtype=np.float64)
    b = E.centred(a) if center else a
    lam, vec = np.linalg.eigh((b + b.T) / 2)
    return lam[::-1], vec[:, ::-1]


def check(phi, got, k, center, tol=TOL, oracle=True, seed=0, maxiter=300):
    """Everything in the module's docstring, for one call's (values, vectors, residual, converged, products)."""
    val, vec, res, conv, m = got
    n = len(phi)
    lam, ref = spectrum(phi, center)
    kk = min(k + 1, n)
    assert np.all(-np.diff(lam[:kk]) > 2 * tol * lam[0]), lam[:kk]              # the premise of the per-rank checks
    assert val.shape == (k,) and vec.shape == (n, k) and res.shape == (k,) and conv.shape == (k,) and conv.dtype == bool
    assert 1 <= m <= min(maxiter, n)
    r = rounding(n, m, val[0])
    assert np.all(np.diff(val) <= 0)
    assert np.all(np.abs(val - lam[:k]) <= res + r), (val - lam[:k], res)
    assert np.all(val <= lam[:k] + r)
    others = np.abs(lam[None, :] - val[:, None])
    others[np.arange(k), np.arange(k)] = np.inf
    gap = others.min(axis=1)
    q = ref[:, :k]
    sine = np.linalg.norm(vec - q * np.einsum("ij,ij->j", q, vec), axis=0)
    assert np.all(sine <= (res + r) / gap), (sine, (res + r) / gap)
    assert np.all(res[conv] <= tol * val[0] + r), (res, conv)
    print("N = %d k = %d center = %s: %d products, largest residual / (tol theta_1) = %.3g, rounding / (tol theta_1) = %.3g" % (
        n, k, center, m, float(np.max(res) / (tol * val[0])), r / (tol * val[0])))
    big = np.argmax(np.abs(vec), axis=0)
    assert np.all(vec[big, np.arange(k)] > 0)
    orth = np.abs(vec.T @ vec - np.eye(k)).max()
    orth_ref = np.abs(q.T @ q - np.eye(k)).max()
    print("  |V^T V - I|_max = %.3g, of eigh's own vectors %.3g" % (orth, orth_ref))
    assert orth <= (m + 2) * max(orth_ref, (n + 2) * U)
    if center:
        assert np.all(np.abs(vec.sum(axis=0)) <= (n + 2) * U * np.sqrt(n))
    if oracle:
        o = E.lanczos(phi, k, center=center, tol=tol, maxiter=maxiter, seed=seed)
        lo, hi = o["steps"][4 * tol], o["steps"][tol / 4]
        assert np.all(conv) and lo is not None, (conv, o["steps"])
        assert lo <= m <= (hi if hi is not None else min(maxiter, n)), (m, o["steps"])
    return m


# ---- geneaJi and unrelated founders -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,center", [(1, False), (2, False), (3, False), (2, True)])
def test_geneaJi(gen, k, center):
    ped = gen.genealogy(gen.geneaJi)
    pl = gen.plan(ped)
    try:
        phi = pl.compute(device=0)
        check(phi, pl.eigen(k, center), k, center)
    finally:
        pl.close()
    got = gen.phiEigen(ped, k=k, center=center, device=0)
    assert np.array_equal(got.pro, gen.pro(ped)) and got.center is center and got.tol == TOL and "PhiEigen" in repr(got)
    assert np.array_equal(got.coordinates, got.vectors * np.sqrt(np.maximum(got.values, 0.0)))


def test_unrelated_founders_break_down_at_every_step(gen):
    """Phi = I / 2 for 70 founders: every step ends in a breakdown, fresh vectors supply the copies of the one eigenvalue."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, _ = synth.random_mating(2000, 50, 3, seed=2)
    founders = ind[(fa == 0) & (mo == 0)][:70]
    assert len(founders) == 70
    pl = gen.plan(gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}), founders)
    try:
        assert np.array_equal(pl.compute(device=0), np.eye(70, dtype=np.float32) / 2)
        val, vec, res, conv, m = pl.eigen(5)
        assert m == 5 and val.tolist() == [0.5] * 5 and np.all(conv)
        assert np.all(res <= rounding(70, 5, 0.5))
        assert np.abs(vec.T @ vec - np.eye(5)).max() <= 7 * 72 * U
        big = np.argmax(np.abs(vec), axis=0)
        assert np.all(vec[big, np.arange(5)] > 0)
        o = E.lanczos(np.eye(70) / 2, 5)
        assert o["products"] == 5 and np.abs(o["vectors"] - vec).max() <= 64 * 72 * U         # the same stream, the same fresh vectors
    finally:
        pl.close()


# ---- genea140 and the synthetic 2,500 -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def genea140_case(gen):
    golden = np.load(GOLDEN140)
    pl = gen.plan(gen.genealogy(gen.genea140))
    assert np.array_equal(pl.compute(device=0), golden)
    yield pl, golden
    pl.close()


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("k", [1, 4, 10])
def test_genea140_against_the_committed_oracle_matrix(genea140_case, k, center):
    pl, golden = genea140_case
    check(golden, pl.eigen(k, center, TOL), k, center)


@pytest.mark.parametrize("center", [False, True])
def test_synthetic_case(synth_case, center):
    pl, phi = synth_case[2], synth_case[3]
    check(phi, pl.eigen(10, center, TOL), 10, center)


def test_maxiter_12_returns_with_consistent_flags(genea140_case):
    pl, golden = genea140_case
    got = pl.eigen(10, False, TOL, maxiter=12)
    val, vec, res, conv, m = got
    assert m == 12 and not np.all(conv)
    r = rounding(140, 12, val[0])
    assert np.all(res[conv] <= TOL * val[0] + r)
    lam = spectrum(golden, False)[0]
    assert np.all(val <= lam[:10] + r) and np.all(np.diff(val) <= 0)
    dist = np.abs(lam[None, :] - val[:, None]).min(axis=1)
    assert np.all(dist <= res + r)                                          # some eigenvalue within the TRUE residual of every pair
    assert np.abs(vec.T @ vec - np.eye(10)).max() <= 14 * 142 * U


# ---- sizes at the kernels' edges ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_sizes_at_the_steps_of_the_kernels(gen, synth_case, n):
    ped, pro, _, full, _ = synth_case
    pl = gen.plan(ped, pro[100:100 + n])
    try:
        phi = pl.compute(device=0)
        assert np.array_equal(phi, full[100:100 + n, 100:100 + n])
        k = min(3, n)
        for center in (False, True) if n > 3 else (False,):
            check(phi, pl.eigen(k, center, TOL), k, center)
    finally:
        pl.close()


# ---- invariances, as bytes ----------------------------------------------------------------------------------------------------------

def test_the_same_call_twice_and_after_a_stale_inf_panel(gen, synth_case):
    """N = 2,498: two padding rows in every vector, which an earlier panel of infinities in the same scratch block filled."""
    ped, pro, _, _, _ = synth_case
    pl = gen.plan(ped, pro[:2498])
    try:
        pl.compute_device(device=0)
        a = pl.eigen(4, True, TOL)
        b = pl.eigen(4, True, TOL)
        with np.errstate(invalid="ignore"):
            assert not np.any(np.isfinite(pl.matmul(np.full((2498, 64), np.inf))))
        c = pl.eigen(4, True, TOL)
        for x, y, z in zip(a[:4], b[:4], c[:4]):
            assert same(x, y) and same(x, z)
        assert a[4] == b[4] == c[4]
        other = pl.eigen(4, True, TOL, seed=1)
        assert not same(other[1], a[1]) and np.abs(other[0] - a[0]).max() <= 2 * TOL * a[0][0]    # another start, the same pairs
    finally:
        pl.close()


def test_phiEigen_of_a_pedigree_gives_the_plan_methods_bytes(gen, synth_case):
    ped, pro, pl, _, _ = synth_case
    got = gen.phiEigen(ped, k=3, center=True, probandIDs=np.concatenate([pro[:7], pro]), device=0)      # duplicates collapse
    ref = pl.eigen(3, True)
    assert same(got.values, ref[0]) and same(got.vectors, ref[1]) and same(got.residual, ref[2]) and same(got.converged, ref[3])
    assert got.products == ref[4] and np.array_equal(got.pro, pro)


# ---- errors -----------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_plan_usable(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(4000, 400, 10, skip_permille=50)
    pl = gen.plan(gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}), pro)
    L, C = gen._capi.lib(), gen._capi
    val, vec, res = np.full(8, -7.0), np.full((400, 8), -7.0), np.full(8, -7.0)
    conv, prod = np.full(8, -7, dtype=np.int32), ctypes.c_int32(-7)

    def call(h, k=3, center=0, tol=TOL, maxiter=300, v=val.ctypes.data_as(DP), w=vec.ctypes.data_as(DP), ldv=8):
        return L.genphi_result_eigen(h, k, center, tol, maxiter, 0, v, w, ldv, res.ctypes.data_as(DP), conv.ctypes.data_as(IP), ctypes.byref(prod))

    def untouched():
        return np.all(val == -7.0) and np.all(vec == -7.0) and np.all(res == -7.0) and np.all(conv == -7) and prod.value == -7

    try:
        with pytest.raises(gen.GenphiDeviceError):                        # no resident result yet
            pl.eigen(3)
        assert call(pl._h) == C.GENPHI_ERR_DEVICE
        phi = pl.compute(device=0)
        sums = pl.result_sums()
        ref = pl.eigen(3)

        def good():
            assert all(same(a, b) for a, b in zip(pl.eigen(3)[:4], ref[:4]))
            assert pl.result_sums() == sums and np.array_equal(pl.result_to_host(), phi)

        assert call(None) == C.GENPHI_ERR_ARG
        for kw in (dict(k=0), dict(k=65), dict(k=-1), dict(tol=-1.0), dict(tol=float("nan")), dict(maxiter=2), dict(maxiter=4097), dict(ldv=2),
                   dict(v=None), dict(w=None)):
            assert call(pl._h, **kw) == C.GENPHI_ERR_ARG, kw
            assert "genphi_result_eigen" in C.last_error()
            assert untouched()
            good()
        # the order of the checks: k before tol before max_iter before the pitch before the pointers
        assert call(pl._h, k=0, tol=-1.0) == C.GENPHI_ERR_ARG and "k = 0" in C.last_error()
        assert call(pl._h, tol=-1.0, maxiter=1) == C.GENPHI_ERR_ARG and "tol" in C.last_error()
        assert call(pl._h, maxiter=1, ldv=1) == C.GENPHI_ERR_ARG and "max_iter" in C.last_error()
        assert call(pl._h, ldv=1, v=None) == C.GENPHI_ERR_ARG and "pitch" in C.last_error()
        for bad in (dict(k=0), dict(k=401), dict(k=65), dict(tol=-1.0), dict(k=5, maxiter=4), dict(maxiter=4097)):
            with pytest.raises(ValueError):
                pl.eigen(**bad)
        with pytest.raises(ValueError):
            gen.phiEigen(gen.genealogy(gen.geneaJi), k=4, device=0)       # k > N = 3
        pl.compute_device(device=0, storage64=True)                       # a Float64 result
        with pytest.raises(ValueError, match="Float32"):
            pl.eigen(3)
        assert call(pl._h) == C.GENPHI_ERR_ARG
        for rows in ((7, 7), (0, 399), (399, 400)):                       # shards, one of them empty
            pl.compute_device(device=0, rows=rows)
            with pytest.raises(ValueError, match="shard"):
                pl.eigen(3)
            assert call(pl._h) == C.GENPHI_ERR_ARG
        pl.compute_device(device=0)
        good()
        pl.release_device()
        with pytest.raises(gen.GenphiDeviceError):
            pl.eigen(3)
        assert call(pl._h) == C.GENPHI_ERR_DEVICE
        assert untouched()                                                # no failed call wrote anything
        pl.compute_device(device=0)
        good()
        assert call(pl._h, k=3, ldv=8) == 0 and prod.value == ref[4]      # a pitch beyond k: the gaps survive
        assert np.array_equal(vec[:, :3], ref[1]) and np.all(vec[:, 3:] == -7.0) and np.array_equal(val[:3], ref[0]) and np.all(val[3:] == -7.0)
    finally:
        pl.close()
