"""genphi_result_matmul / PhiPlan.matmul / gen.phiMatmul on the GPU (include/genphi.h).

Exact cases carry no tolerance: every Float32 kinship is a dyadic number, so with an integer X every partial sum of an entry is exact in
Float64 while max_i sum_j |Phi_ij| . max|x| . 2^q < 2^53 (2^-q the smallest unit of any entry) -- exact_condition asserts that on the
host copy before a test relies on it -- and the product then equals phi.astype(float64) @ X in ANY order of the additions.  A general
X is held to the a-priori bound of N fused terms in any order, (N + 2) 2^-53 (|Phi| |X|), against a numpy.longdouble product.  The
invariances the header states (same call, one column of many, row shards, stale scratch) are compared as bytes."""
import ctypes
import os

import numpy as np
import pytest

from test_phi_over_gpu import synth_case                    # noqa: F401  (the 2,500 probands of the phiOver tests: a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN140 = os.path.join(ROOT, "tests", "golden", "genea140_phi_oracle.npy")
U = 2.0 ** -53
KS = [1, 2, 3, 5, 8, 9, 16, 17, 63, 64]
# csrc/matmul.hip, by the kernel's names: rows of a workgroup = kMmWaves x kMmRowsWide / kMmRowsNarrow; columns of a step; columns
# staged between two barriers (kMmChunkWide16, kMmChunkWide8, kMmChunkNarrow); column tiles of the forms
ROW_BLOCKS = (4 * 4, 4 * 8)
STEP = 256
CHUNKS = (256, 512, 1024)
TILES = (1, 2, 4, 8, 16)
DP = ctypes.POINTER(ctypes.c_double)


def unit_bits(phi):
    """q: 2^-q is the smallest unit of any entry of the Float32 matrix (every entry is an integer multiple of it)."""
    v = np.asarray(phi, dtype=np.float32).ravel()
    v = v[v != 0]
    if len(v) == 0:
        return 0
    mant, exp = np.frexp(v.astype(np.float64))                   # v = mant 2^exp, mant 2^24 an integer
    m = (mant * 2.0 ** 24).astype(np.int64)
    assert np.array_equal(m.astype(np.float64) * 2.0 ** (exp.astype(np.float64) - 24), v.astype(np.float64))
    low = np.log2((m & -m).astype(np.float64)).astype(np.int64)  # trailing zeros
    return int(max(0, -(exp.astype(np.int64) - 24 + low).min()))


def exact_condition(phi, X):
    """Asserts that phi @ X is exact in Float64 in any order: integer X and max_i sum_j |Phi_ij| max|x| 2^q < 2^53.  Returns log2 of it."""
    X = np.asarray(X, dtype=np.float64)
    assert np.all(np.isfinite(X)) and np.array_equal(X, np.rint(X))
    q = unit_bits(phi)
    rows = np.abs(np.asarray(phi, dtype=np.float64)).sum(axis=1).max() if np.size(phi) else 0.0
    size = float(rows) * max(float(np.abs(X).max()) if X.size else 0.0, 1.0) * 2.0 ** q
    assert size < 2.0 ** 53, (q, size)
    return np.log2(max(size, 1.0))


def int_panel(n, k, bound, seed):
    return np.random.default_rng(seed).integers(-bound, bound + 1, size=(n, k)).astype(np.float64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- geneaJi ------------------------------------------------------------------------------------------------------------------

def test_geneaJi_row_sums_and_the_matrix_itself(gen):
    ped = gen.genealogy(gen.geneaJi)
    pl = gen.plan(ped)
    try:
        phi = pl.compute(device=0).astype(np.float64)
        exact_condition(phi, np.ones(3))
        got = pl.matmul(np.ones(3))
        assert got.shape == (3,) and got.dtype == np.float64 and np.array_equal(got, phi.sum(axis=1))
        assert np.array_equal(pl.matmul(np.eye(3)), phi)
        assert np.array_equal(pl.matmul(np.ones((3, 1))), phi.sum(axis=1)[:, None])
    finally:
        pl.close()
    assert np.array_equal(gen.phiMatmul(ped, np.eye(3), device=0), phi)
    got = gen.phiMatmul(ped, [1.0, 2.0, 4.0], probandIDs=[29, 2, 29, 1], device=0)          # duplicates collapse: rows [29, 2, 1]
    assert np.array_equal(got, phi[[2, 1, 0]][:, [2, 1, 0]] @ np.array([1.0, 2.0, 4.0]))


# ---- genea140 and the synthetic 2,500 -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def genea140_case(gen):
    golden = np.load(GOLDEN140)
    pl = gen.plan(gen.genealogy(gen.genea140))
    pl.compute_device(device=0)
    X = int_panel(140, 130, 1000, 140)
    assert exact_condition(golden, X) < 42.0 and unit_bits(golden) == 32
    yield pl, golden, X, golden.astype(np.float64) @ X
    pl.close()


@pytest.fixture(scope="module")
def synth_exact(synth_case):
    phi = synth_case[3]
    X = int_panel(2500, 130, 2 ** 20, 2500)
    assert exact_condition(phi, X) < 42.0 and unit_bits(phi) == 19
    return X, phi.astype(np.float64) @ X


@pytest.mark.parametrize("k", KS)
def test_genea140_against_the_committed_oracle_matrix(genea140_case, k):
    pl, _, X, ref = genea140_case
    assert same(pl.matmul(X[:, :k]), np.ascontiguousarray(ref[:, :k]))


def test_genea140_more_than_64_columns(genea140_case):
    pl, _, X, ref = genea140_case
    assert same(pl.matmul(X), ref)
    assert same(pl.matmul(X[:, 0]), np.ascontiguousarray(ref[:, 0]))


@pytest.mark.parametrize("k", KS)
def test_synthetic_case(synth_case, synth_exact, k):
    pl, (X, ref) = synth_case[2], synth_exact
    assert same(pl.matmul(X[:, :k]), np.ascontiguousarray(ref[:, :k]))


def test_synthetic_case_more_than_64_columns(synth_case, synth_exact):
    pl, (X, ref) = synth_case[2], synth_exact
    assert same(pl.matmul(X), ref)


def test_phiMatmul_of_a_pedigree_gives_the_plan_methods_bytes(gen, synth_case, synth_exact):
    ped, pro, pl, _, _ = synth_case
    X, ref = synth_exact
    assert same(gen.phiMatmul(ped, X[:, :5], probandIDs=pro, device=0), pl.matmul(X[:, :5]))
    g = np.random.default_rng(5).standard_normal((2500, 3))                                     # (not exact: the same bytes all the same)
    assert same(gen.phiMatmul(ped, g, probandIDs=pro, device=0), pl.matmul(g))
    twice = np.concatenate([pro[:7], pro])                                                     # duplicates collapse
    assert same(gen.phiMatmul(ped, X[:, 0], probandIDs=twice, device=0), np.ascontiguousarray(ref[:, 0]))


# ---- edges ------------------------------------------------------------------------------------------------------------------------

EDGES = sorted(set([1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1027] + [b + d for b in ROW_BLOCKS + (STEP,) + CHUNKS for d in (-1, 0, 1)]))


@pytest.mark.parametrize("n", EDGES)
def test_row_block_and_chunk_edges(gen, synth_case, n):
    ped, pro, _, _, _ = synth_case
    pl = gen.plan(ped, pro[100:100 + n])
    try:
        phi = pl.compute(device=0)
        assert phi.shape == (n, n)
        X = int_panel(n, 17, 2 ** 20, n)
        exact_condition(phi, X)
        ref = phi.astype(np.float64) @ X
        for k in (1, 2, 3, 8, 9, 17):                                                          # every column tile, and two tiles of 16
            assert same(pl.matmul(X[:, :k]), np.ascontiguousarray(ref[:, :k])), k
    finally:
        pl.close()


def test_pitches_beyond_k_and_the_gaps_of_y_survive(gen, synth_case, synth_exact):
    pl, (X, ref) = synth_case[2], synth_exact
    L = gen._capi.lib()
    for k, ldx, ldy in ((1, 3, 2), (5, 130, 7), (17, 130, 64), (64, 65, 130)):
        x = np.full((2500, ldx), np.inf)                                                       # the gaps of x are never read
        x[:, :k] = X[:, :k]
        y = np.full((2500, ldy), -7.0)
        rows = ctypes.c_int64(-1)
        assert L.genphi_result_matmul(pl._h, k, x.ctypes.data_as(DP), ldx, y.ctypes.data_as(DP), ldy, ctypes.byref(rows)) == 0
        assert rows.value == 2500 and np.array_equal(y[:, :k], ref[:, :k]) and np.all(y[:, k:] == -7.0)


# ---- a general X ------------------------------------------------------------------------------------------------------------------

def test_standard_normal_panel_within_the_a_priori_bound(synth_case):
    pl, phi = synth_case[2], synth_case[3]
    n = len(phi)
    X = np.random.default_rng(20261018).standard_normal((n, 17))
    got = pl.matmul(X)
    ref = phi.astype(np.longdouble) @ X.astype(np.longdouble)
    bound = (n + 2) * U * (np.abs(phi.astype(np.float64)) @ np.abs(X))
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    print("largest error / bound: %.4g (numpy's own Float64 product: %.4g)" % ((err / bound).max(), (np.abs((phi.astype(np.float64) @ X).astype(np.longdouble) - ref).astype(np.float64) / bound).max()))
    assert np.all(err <= bound)
    one = pl.matmul(X[:, 4])
    assert same(one, np.ascontiguousarray(got[:, 4]))


def test_ieee_semantics_zero_times_inf_is_nan(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, _ = synth.random_mating(600, 50, 5, seed=2)
    founders = ind[(fa == 0) & (mo == 0)][:5]                                                   # unrelated: Phi = I / 2, zeros elsewhere
    pl = gen.plan(gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}), founders)
    try:
        phi = pl.compute(device=0).astype(np.float64)
        assert np.array_equal(phi, np.eye(5) / 2)
        x = np.array([1.0, np.inf, -2.0, 0.0, -np.inf])
        with np.errstate(invalid="ignore"):
            ref = phi @ x
        assert np.isnan(ref).sum() == 5                                                        # every row meets 0 x inf, as in numpy
        assert np.array_equal(np.isnan(pl.matmul(x)), np.isnan(ref))
        x[4] = 3.0
        with np.errstate(invalid="ignore"):
            ref = phi @ x
        got = pl.matmul(x)
        assert np.isnan(ref).sum() == 4 and np.array_equal(np.isnan(got), np.isnan(ref)) and got[1] == np.inf
    finally:
        pl.close()


# ---- invariances, as bytes ----------------------------------------------------------------------------------------------------------

def test_the_same_call_twice_and_every_column_alone(synth_case):
    pl = synth_case[2]
    X = np.random.default_rng(64).standard_normal((2500, 64)) * np.exp(np.random.default_rng(65).uniform(-20, 20, size=(2500, 64)))
    a, b = pl.matmul(X), pl.matmul(X)
    assert same(a, b)
    for c in range(64):
        assert same(pl.matmul(X[:, c]), np.ascontiguousarray(a[:, c])), c
    for k in (2, 3, 8, 9, 17):                                                                 # a column in every kernel form
        assert same(pl.matmul(X[:, :k]), np.ascontiguousarray(a[:, :k])), k


def test_row_shards_stack_to_the_full_result(synth_case):
    pl, phi = synth_case[2], synth_case[3]
    n = len(phi)
    X = np.random.default_rng(7).standard_normal((n, 9))
    full = pl.matmul(X)
    try:
        parts = []
        for rows in ((0, 1111), (1111, 1111), (1111, 1790), (1790, n)):                         # a split off every alignment, one shard empty
            pl.compute_device(device=0, rows=rows)
            parts.append(pl.matmul(X))
        assert [p.shape for p in parts] == [(1111, 9), (0, 9), (679, 9), (710, 9)]
        assert same(np.concatenate(parts), full)
        pl.compute_device(device=0, rows=(n - 1, n))
        assert same(pl.matmul(X), np.ascontiguousarray(full[n - 1:]))
        assert same(pl.matmul(X[:, 3]), np.ascontiguousarray(full[n - 1:, 3]))
    finally:
        pl.compute_device(device=0)                                          # (the module's plan holds the full result again)
    assert same(pl.matmul(X), full)


def test_a_stale_inf_in_the_scratch_block_does_not_meet_the_padding(gen, synth_case, synth_exact):
    """N = 2,498: the device copy of X has two padding rows (2,498 and 2,499) that an earlier, larger panel of infinities filled."""
    ped, pro, _, _, _ = synth_case
    pl = gen.plan(ped, pro[:2498])
    try:
        phi = pl.compute(device=0)
        with np.errstate(invalid="ignore"):
            bad = pl.matmul(np.full((2498, 64), np.inf))
        assert not np.any(np.isfinite(bad))
        for k in (1, 3, 8, 17, 64):
            X = int_panel(2498, k, 2 ** 20, k)
            exact_condition(phi, X)
            assert same(pl.matmul(X), phi.astype(np.float64) @ X), k
            with np.errstate(invalid="ignore"):
                pl.matmul(np.full((2498, 64), np.inf))
    finally:
        pl.close()


# ---- errors -----------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_plan_usable(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(4000, 400, 10, skip_permille=50)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    L, C = gen._capi.lib(), gen._capi
    X = int_panel(400, 64, 1000, 400)
    y = np.full((400, 64), -7.0)
    rows = ctypes.c_int64(-7)
    px, py = X.ctypes.data_as(DP), y.ctypes.data_as(DP)

    def call(h, k, x, ldx, yy, ldy):
        return L.genphi_result_matmul(h, k, x, ldx, yy, ldy, ctypes.byref(rows))

    try:
        with pytest.raises(gen.GenphiDeviceError):                        # no resident result yet
            pl.matmul(X)
        assert call(pl._h, 64, px, 64, py, 64) == C.GENPHI_ERR_DEVICE
        phi = pl.compute(device=0)
        exact_condition(phi, X)
        ref = phi.astype(np.float64) @ X
        sums = pl.result_sums()

        def good():
            assert same(pl.matmul(X), ref)
            assert pl.result_sums() == sums and np.array_equal(pl.result_to_host(), phi)

        good()
        assert call(None, 64, px, 64, py, 64) == C.GENPHI_ERR_ARG
        for k, x, ldx, yy, ldy in ((0, px, 64, py, 64), (65, px, 65, py, 65), (-1, px, 64, py, 64), (3, None, 64, py, 64), (3, px, 64, None, 64),
                                   (3, px, 2, py, 64), (3, px, 64, py, 2)):
            assert call(pl._h, k, x, ldx, yy, ldy) == C.GENPHI_ERR_ARG, (k, ldx, ldy)
            assert "genphi_result_matmul" in C.last_error()
            good()
        for bad in (np.ones(399), np.ones((401, 2)), np.ones((2, 400)), np.ones((400, 2, 2))):
            with pytest.raises(ValueError):
                pl.matmul(bad)
        pl.compute_device(device=0, storage64=True)                       # a Float64 result
        with pytest.raises(ValueError, match="Float32"):
            pl.matmul(X)
        assert call(pl._h, 64, px, 64, py, 64) == C.GENPHI_ERR_ARG
        pl.compute_device(device=0, rows=(7, 7))                          # an empty shard: OK, nothing written, 0 rows
        assert call(pl._h, 64, px, 64, None, 64) == 0 and rows.value == 0
        rows.value = -7
        assert pl.matmul(X).shape == (0, 64) and pl.matmul(X[:, 0]).shape == (0,)
        pl.compute_device(device=0)
        good()
        pl.release_device()
        with pytest.raises(gen.GenphiDeviceError):
            pl.matmul(X)
        assert call(pl._h, 64, px, 64, py, 64) == C.GENPHI_ERR_DEVICE
        assert np.all(y == -7.0) and rows.value == -7                     # no failed call wrote anything
        pl.compute_device(device=0)
        good()
    finally:
        pl.close()
