"""genphi_result_over / PhiPlan.phi_over / gen.phiOver on the GPU against tests/phi_over_oracle.py, on the host matrix of the same
plan.  The selection only compares and copies, so every check is np.array_equal (values as bit patterns): no tolerance anywhere."""
import ctypes
import math

import numpy as np
import pytest

import phi_over_oracle as PO

pytestmark = pytest.mark.gpu


def _check(pl, phi_rows, t, row_begin=0):
    """phi_over(t) of the plan's resident rows (phi_rows = those rows on the host) is the oracle's list; returns it."""
    got = pl.phi_over(t)
    ref = PO.over_numpy(phi_rows, t, row_begin=row_begin)
    print("threshold %r, rows [%d, %d): %d pairs (oracle %d)" % (t, row_begin, row_begin + len(phi_rows), len(got[0]), len(ref[0])))
    assert PO.same(got, ref)
    assert pl.count_over(t) == len(ref[0])
    return got


def _distinct_off_diagonal(phi):
    """The distinct values right of the diagonal, largest first."""
    return np.unique(phi[np.triu_indices(len(phi), 1)])[::-1]


# ---- geneaJi ------------------------------------------------------------------------------------------------------------------

def test_geneaJi(gen):
    ped = gen.genealogy(gen.geneaJi)
    assert gen.pro(ped).tolist() == [1, 2, 29]
    phi = gen.phi(ped, device=0)
    pl = gen.plan(ped)
    try:
        assert np.array_equal(pl.compute(device=0), phi)
        r, c, v = _check(pl, phi, 0.0)
        assert r.tolist() == [0, 0, 1] and c.tolist() == [1, 2, 2] and v.tolist() == [phi[0, 1], phi[0, 2], phi[1, 2]]
        top = float(max(phi[0, 1], phi[0, 2], phi[1, 2]))
        assert len(_check(pl, phi, top)[0]) >= 1
        assert len(_check(pl, phi, float(np.nextafter(np.float32(top), np.float32(1))))[0]) == 0
        assert PO.same(PO.over(phi, 0.0), (r, c, v))                            # (the loop form of the oracle, too)
    finally:
        pl.close()
    got = gen.phiOver(ped, 0.0, device=0)
    assert len(got) == 3 and got.pro1.tolist() == [1, 1, 2] and got.pro2.tolist() == [2, 29, 29]
    assert got.row.tolist() == [0, 0, 1] and got.col.tolist() == [1, 2, 2] and got.kinship.tolist() == [phi[0, 1], phi[0, 2], phi[1, 2]]
    assert "3 pairs" in repr(got)
    got = gen.phiOver(ped, 0.0, probandIDs=[29, 2, 29, 1], device=0)            # duplicates collapse: positions in [29, 2, 1]
    assert got.pro1.tolist() == [29, 29, 2] and got.pro2.tolist() == [2, 1, 1]
    assert got.kinship.tolist() == [phi[1, 2], phi[0, 2], phi[0, 1]]
    host = gen.phiOver(phi, top, probandIDs=[1, 2, 29])                          # the host form gives the same answer
    dev = gen.phiOver(ped, top, device=0)
    assert PO.same((host.row, host.col, host.kinship), (dev.row, dev.col, dev.kinship)) and np.array_equal(host.pro2, dev.pro2)
    assert len(gen.phiOver(ped, 1.0, device=0)) == 0


# ---- the 2,500 probands of test_group_sums_gpu.py ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def synth_case(gen):
    """(pedigree, proband IDs, plan with the full result resident, host matrix, its distinct off-diagonal values, largest first).
    2,500 probands: ld = 2,560, so 60 zero padding columns that a threshold <= 0 must not list; rows of 3 tiles down to none."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(30_000, 2_500, 10, skip_permille=50)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    phi = pl.compute(device=0)
    assert phi.shape == (2500, 2500) and pl.result_device()[1] == 2560
    yield ped, np.asarray(pro, dtype=np.int64), pl, phi, _distinct_off_diagonal(phi)
    pl.close()


@pytest.mark.parametrize("t", [0.0, -1.0, -math.inf])
def test_every_pair_and_no_padding_column(synth_case, t):
    _, _, pl, phi, _ = synth_case
    r, c, v = _check(pl, phi, t)
    assert len(r) == 3_123_750 == 2500 * 2499 // 2 and int(c.max()) == 2499 and np.all(r < c)


def test_nothing_above_the_maximum(synth_case):
    _, _, pl, phi, distinct = synth_case
    for t in (math.inf, float(np.nextafter(distinct[0], np.float32(np.inf))), 1.0e300):
        assert all(len(a) == 0 for a in _check(pl, phi, t))
    assert len(_check(pl, phi, float(distinct[0]))[0]) >= 1                     # the maximum itself is listed: >=


@pytest.mark.parametrize("rank", [10, 1_000, 100_000])
def test_ties_at_the_edge_of_the_threshold(synth_case, rank):
    """The rank-th largest distinct off-diagonal value as the threshold: every entry equal to it is listed, and a threshold one
    Float64 step above it (between two Float32 values) lists none of them.  This pedigree has 9,331 distinct off-diagonal
    kinships (CPU oracle), so no 100,000th distinct one: that case takes the 100,000th largest off-diagonal ENTRY instead, repeats
    counted, which is again a value of the data with ties at the edge."""
    _, _, pl, phi, distinct = synth_case
    if rank <= len(distinct):
        t = float(distinct[rank - 1])
    else:
        t = float(np.sort(phi[np.triu_indices(len(phi), 1)])[::-1][rank - 1])
    r, c, v = _check(pl, phi, t)
    ties = int(np.count_nonzero(v == np.float32(t)))
    assert ties >= 1 and np.all(v >= np.float32(t))
    above = _check(pl, phi, float(np.nextafter(t, math.inf)))
    assert len(above[0]) == len(r) - ties
    if rank == 1_000:
        assert 0 < len(r) < 3_123_750 // 2


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_every_alignment_of_a_rows_start_and_end(gen, synth_case, n):
    ped, pro, _, _, _ = synth_case
    pl = gen.plan(ped, pro[100:100 + n])
    try:
        phi = pl.compute(device=0)
        assert phi.shape == (n, n)
        assert len(_check(pl, phi, 0.0)[0]) == n * (n - 1) // 2
        if n >= 2:
            distinct = _distinct_off_diagonal(phi)
            got = _check(pl, phi, float(distinct[len(distinct) // 3]))
            assert 0 < len(got[0]) <= n * (n - 1) // 2
    finally:
        pl.close()


def test_row_shards_concatenate_and_a_recomputed_result_is_counted_again(synth_case):
    _, _, pl, phi, distinct = synth_case
    n = len(phi)
    t = float(distinct[999])
    full = _check(pl, phi, t)
    try:
        parts = []
        for rows in ((0, 1111), (1111, n)):
            pl.compute_device(device=0, rows=rows)
            parts.append(_check(pl, phi[rows[0]:rows[1]], t, row_begin=rows[0]))
            _check(pl, phi[rows[0]:rows[1]], 0.0, row_begin=rows[0])
        assert PO.same(tuple(np.concatenate(x) for x in zip(*parts)), full)
        for rows in ((n - 1, n), (0, 1)):
            pl.compute_device(device=0, rows=rows)
            got = _check(pl, phi[rows[0]:rows[1]], 0.0, row_begin=rows[0])
            assert len(got[0]) == (0 if rows[0] else n - 1)
        # two shards of the same number of rows, the same threshold: counts kept from the first would fit the second
        pl.compute_device(device=0, rows=(0, 1250))
        first = pl.count_over(t)
        pl.compute_device(device=0, rows=(1250, n))
        second = pl.count_over(t)
        assert first == len(PO.over_numpy(phi[:1250], t)[0]) and second == len(PO.over_numpy(phi[1250:], t, row_begin=1250)[0])
        assert first != second and first + second == len(full[0])
        _check(pl, phi[1250:], t, row_begin=1250)
    finally:
        pl.compute_device(device=0)                                          # (the module's plan holds the full result again)
    assert PO.same(_check(pl, phi, t), full)


def test_cap_and_null_arrays(gen, synth_case):
    _, _, pl, phi, distinct = synth_case
    L, i32p, f32p = gen._capi.lib(), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    t = float(distinct[999])
    ref = PO.over_numpy(phi, t)
    m = len(ref[0])
    assert m > 1

    def call(cap, want=(True, True, True)):
        r, c, v = np.full(m, -7, np.int32), np.full(m, -7, np.int32), np.full(m, -7.0, np.float32)
        got = ctypes.c_int64(-1)
        rc = L.genphi_result_over(pl._h, t, cap, r.ctypes.data_as(i32p) if want[0] else None, c.ctypes.data_as(i32p) if want[1] else None,
                                  v.ctypes.data_as(f32p) if want[2] else None, ctypes.byref(got))
        assert rc == 0 and got.value == m
        return r, c, v

    for cap in (m - 1, 0):                                                   # too small: the sentinels stay
        r, c, v = call(cap)
        assert np.all(r == -7) and np.all(c == -7) and np.all(v == -7.0)
    assert PO.same(call(m), ref)
    assert PO.same(call(m + 5), ref)
    for k in range(3):                                                       # any single array may be NULL, or any two
        for want in ([j != k for j in range(3)], [j == k for j in range(3)]):
            out = call(m, want)
            for j in range(3):
                assert np.array_equal(out[j], ref[j]) if want[j] else np.all(out[j] == -7)
    assert L.genphi_result_over(pl._h, t, m, None, None, None, None) == 0    # count only, and nowhere to put the count


def test_the_same_call_gives_the_same_bytes(synth_case):
    _, _, pl, phi, distinct = synth_case
    for t in (float(distinct[len(distinct) // 2]), 0.0):
        a, b = pl.phi_over(t), pl.phi_over(t)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and pl.count_over(t) == len(a[0])


def test_phiOver_of_a_pedigree_names_the_probands(gen, synth_case):
    ped, pro, _, phi, distinct = synth_case
    t = float(distinct[9])
    got = gen.phiOver(ped, t, probandIDs=pro, device=0)
    ref = PO.over_numpy(phi, t)
    assert PO.same((got.row, got.col, got.kinship), ref) and np.array_equal(got.pro1, pro[ref[0]]) and np.array_equal(got.pro2, pro[ref[1]])


# ---- genea140 -------------------------------------------------------------------------------------------------------------------

def test_genea140_thresholds(gen):
    ped = gen.genealogy(gen.genea140)
    pl = gen.plan(ped)
    try:
        phi = pl.compute(device=0)
        assert phi.shape == (140, 140)
        counts = [len(_check(pl, phi, 2.0 ** -e)[0]) for e in range(4, 13)]
        assert counts == sorted(counts) and counts[0] < counts[-1]
        assert PO.same(pl.phi_over(2.0 ** -8), PO.over(phi, 2.0 ** -8))
    finally:
        pl.close()


# ---- errors -----------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_plan_usable(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(4000, 400, 10, skip_permille=50)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    L, C = gen._capi.lib(), gen._capi
    n = ctypes.c_int64()

    def c_call(t, cap=0):
        return L.genphi_result_over(pl._h, t, cap, None, None, None, ctypes.byref(n))

    try:
        with pytest.raises(gen.GenphiDeviceError):                        # no resident result yet
            pl.phi_over(0.01)
        assert c_call(0.01) == C.GENPHI_ERR_DEVICE
        phi = pl.compute(device=0)
        distinct = _distinct_off_diagonal(phi)
        t = float(distinct[len(distinct) // 4])

        def good():
            _check(pl, phi, t)
            assert np.array_equal(pl.result_to_host(), phi)

        good()
        with pytest.raises(ValueError):
            pl.phi_over(math.nan)
        assert c_call(math.nan) == C.GENPHI_ERR_ARG
        good()
        assert c_call(t, -1) == C.GENPHI_ERR_ARG
        good()
        pl.compute_device(device=0, storage64=True)                       # a Float64 result
        with pytest.raises(ValueError, match="Float32"):
            pl.phi_over(t)
        with pytest.raises(ValueError, match="Float32"):
            pl.count_over(t)
        assert c_call(t) == C.GENPHI_ERR_ARG
        pl.compute_device(device=0)
        good()
        pl.release_device()
        with pytest.raises(gen.GenphiDeviceError):
            pl.phi_over(t)
        assert c_call(t) == C.GENPHI_ERR_DEVICE
        pl.compute_device(device=0)
        good()
    finally:
        pl.close()
