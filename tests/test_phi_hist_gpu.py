"""genphi_result_hist / genphi_result_select, PhiPlan.hist / select / count_pairs and gen.phiHist / gen.phiQuantile on the GPU against
tests/phi_hist_oracle.py on the host matrix of the same plan.  Counting and selecting only compare and add integers, so every check is
np.array_equal (selected values as bit patterns): no tolerance anywhere."""
import ctypes
import math
import os

import numpy as np
import pytest

import phi_hist_oracle as HO
from test_phi_over_gpu import synth_case                    # noqa: F401  (the 2,500 probands of the phiOver tests: a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PAIRS = 2500 * 2499 // 2


def _check(pl, phi_rows, edges, labels=None, g=None, row_begin=0):
    """hist of the plan's resident rows (phi_rows = those rows on the host) is the oracle's; returns it."""
    got = pl.hist(edges, labels, g)
    ref = HO.hist(phi_rows, edges, labels, g, row_begin=row_begin)
    print("%d edges, %s, rows [%d, %d): %d pairs (oracle %d)" % (len(edges), "no groups" if labels is None else "%d groups" % g, row_begin,
                                                                  row_begin + len(phi_rows), HO.total(*got), HO.total(*ref)))
    assert HO.same(got, ref)
    return got


def _check_select(pl, phi_rows, ranks, row_begin=0):
    got = pl.select(ranks)
    ref = HO.select(phi_rows, ranks, row_begin=row_begin)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (ranks, got, ref)
    return got


def _upper(phi):
    return phi[np.triu_indices(len(phi), 1)]


# ---- geneaJi ------------------------------------------------------------------------------------------------------------------

def test_geneaJi(gen):
    ped = gen.genealogy(gen.geneaJi)
    phi = gen.phi(ped, device=0)
    pl = gen.plan(ped)
    try:
        pl.compute_device(device=0)
        c, b, a = _check(pl, phi, [0.0, 1.0])
        assert c.tolist() == [3] and b == 0 and a == 0 and pl.count_pairs() == 3
        vals = np.unique(_upper(phi)).astype(np.float64)
        edges = vals if len(vals) > 1 else np.array([vals[0], vals[0] + 1.0])
        c, b, a = _check(pl, phi, edges)                                    # edges at the values themselves
        assert HO.same((c, b, a), HO.hist_loop(phi, edges)) and c.sum() + b + a == 3 and b == 0 and a == 0
        _check_select(pl, phi, [0, 1, 2])
    finally:
        pl.close()
    edges = np.linspace(0.0, 0.5, 9)
    dev, host = gen.phiHist(ped, bins=8, device=0), gen.phiHist(phi, bins=8)
    assert np.array_equal(dev.edges, edges) and HO.same((dev.counts, dev.below, dev.above), (host.counts, host.below, host.above))
    assert dev.n_pairs == host.n_pairs == 3 and "3 pairs" in repr(dev)
    dup = gen.phiHist(ped, bins=8, probandIDs=[29, 2, 29, 1], device=0)     # duplicates collapse
    assert HO.same((dup.counts, dup.below, dup.above), (host.counts, host.below, host.above)) and dup.n_pairs == 3
    g = gen.phiHist(ped, bins=8, groups={1: "a", 2: "b", 29: "a"}, device=0)
    gh = gen.phiHist(phi, bins=8, groups={1: "a", 2: "b", 29: "a"}, probandIDs=[1, 2, 29])
    assert g.names == ["a", "b"] and g.sizes.tolist() == [2, 1] and g.n_pairs == 3
    assert HO.same((g.counts, g.below, g.above), (gh.counts, gh.below, gh.above))
    q = [0.0, 0.5, 0.75, 1.0]
    assert np.array_equal(gen.phiQuantile(ped, q, device=0), gen.phiQuantile(phi, q))
    assert np.array_equal(gen.phiQuantile(ped, q, probandIDs=[29, 2, 29, 1], device=0), gen.phiQuantile(phi, q))


# ---- the 2,500 probands ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sorted_upper(synth_case):
    return np.sort(_upper(synth_case[3]))


def test_no_padding_column_and_no_diagonal(synth_case):
    """60 padding zeros per row and a diagonal of 1/2 or more: either would show in the zero bin or in the total."""
    _, _, pl, phi, _ = synth_case
    tiny = float(np.nextafter(np.float64(0.0), 1.0))
    c, b, a = _check(pl, phi, [0.0, tiny, 1.0])
    assert c[0] == int(np.count_nonzero(_upper(phi) == 0)) and c.sum() == N_PAIRS and b == 0 and a == 0 and pl.count_pairs() == N_PAIRS


@pytest.mark.parametrize("bins", [1, 64, 1000, 4096])
def test_uniform_bins(synth_case, bins):
    _, _, pl, phi, _ = synth_case
    c, b, a = _check(pl, phi, np.linspace(0.0, 0.5, bins + 1))
    assert c.sum() + b + a == N_PAIRS and b == 0
    c, b, a = _check(pl, phi, np.linspace(2.0 ** -9, 2.0 ** -4, bins + 1))  # the zeros are below, close relatives above
    assert b > 0 and c.sum() + b + a == N_PAIRS


def test_ties_at_edges(synth_case, sorted_upper):
    _, _, pl, phi, distinct = synth_case
    asc = distinct[::-1].astype(np.float64)                                 # the distinct off-diagonal values, ascending
    assert len(asc) > 2000
    on = np.array([asc[9], asc[999], asc[len(asc) // 2]])                   # the 10th, the 1,000th and the median distinct value
    c, _, _ = _check(pl, phi, np.concatenate([[0.0], on, [1.0]]))
    assert c.sum() == N_PAIRS and all(c > 0)
    above = np.nextafter(on, math.inf)                                      # one Float64 step above: between two Float32 values
    c2, _, _ = _check(pl, phi, np.concatenate([[0.0], above, [1.0]]))
    ties = [int(np.count_nonzero(sorted_upper == np.float32(v))) for v in on]
    assert all(t >= 1 for t in ties) and c2[0] == c[0] + ties[0] and c2[-1] == c[-1] - ties[-1]
    _check(pl, phi, np.sort(np.concatenate([on, above])))                   # bins that hold exactly one value each, and outer pairs
    _check(pl, phi, 2.0 ** np.arange(-30.0, 1.0))                           # non-uniform: 2^-30 .. 1
    c, b, a = _check(pl, phi, [-math.inf, 0.0, float(asc[asc > 0][0]), 0.25, math.inf])
    assert b == 0 and a == 0 and c[0] == 0 and c.sum() == N_PAIRS
    c, b, a = _check(pl, phi, [-math.inf, math.inf])
    assert c.tolist() == [N_PAIRS]
    c, b, a = _check(pl, phi, [float(distinct[0]), 1.0])                    # the largest value opens the only bin
    assert c[0] >= 1 and b == N_PAIRS - c[0]
    c, b, a = _check(pl, phi, [0.0, float(distinct[0])])                    # ... and closes it
    assert a == 0 and c[0] == N_PAIRS


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_every_alignment_of_a_rows_start_and_end(gen, synth_case, n):
    ped, pro, _, _, _ = synth_case
    pl = gen.plan(ped, pro[100:100 + n])
    try:
        phi = pl.compute(device=0)
        assert phi.shape == (n, n)
        n_pairs = n * (n - 1) // 2
        c, b, a = _check(pl, phi, np.linspace(0.0, 2.0 ** -5, 8))
        assert c.sum() + b + a == n_pairs == pl.count_pairs()
        if n == 1:
            assert not c.any()
            with pytest.raises(ValueError):
                pl.select([0])
        else:
            _check_select(pl, phi, [0, n_pairs // 2, n_pairs - 1])
    finally:
        pl.close()


def _patterns(n):
    two_runs = np.where(np.arange(n) < n // 3, 1, 0).astype(np.int32)
    inter = (np.arange(n) % 3).astype(np.int32)
    inter[::5] = -1
    many = ((np.arange(n) * 7) % 256).astype(np.int32)
    many[3::11] = -1
    return {"two runs": (two_runs, 2, 64), "interleaved": (inter, 3, 64), "one group": (np.zeros(n, dtype=np.int32), 1, 64),
            "all unlabelled": (np.full(n, -1, dtype=np.int32), 2, 64), "256 groups x 64 bins": (many, 256, 64)}


@pytest.mark.parametrize("pattern", ["two runs", "interleaved", "one group", "all unlabelled", "256 groups x 64 bins"])
def test_groups(synth_case, pattern):
    _, _, pl, phi, _ = synth_case
    labels, g, bins = _patterns(len(phi))[pattern]
    assert g * bins <= 16384 and (pattern != "256 groups x 64 bins" or g * bins == 16384)
    edges = np.linspace(0.0, 2.0 ** -4, bins + 1)
    c, b, a = _check(pl, phi, edges, labels, g)
    assert c.shape == (g, g, bins) and np.array_equal(c, np.transpose(c, (1, 0, 2))) and np.array_equal(b, b.T) and np.array_equal(a, a.T)
    keep = np.nonzero(labels >= 0)[0]
    upper = np.triu(np.ones((g, g), dtype=bool))
    flat = HO.hist(phi[np.ix_(keep, keep)], edges)                          # the ungrouped histogram of the labelled pairs
    assert np.array_equal(c[upper].sum(axis=0), flat[0]) and b[upper].sum() == flat[1] and a[upper].sum() == flat[2]
    if pattern == "all unlabelled":
        assert HO.total(c, b, a) == 0
    if pattern == "one group":
        plain = pl.hist(edges)
        assert np.array_equal(c[0, 0], plain[0]) and b[0, 0] == plain[1] and a[0, 0] == plain[2]


def test_genea140_populations(gen):
    groups = gen._pop(os.path.join(ROOT, "tests", "golden", "pop140.csv"))
    ped = gen.genealogy(gen.genea140)
    got = gen.phiHist(ped, bins=64, range=(0.0, 0.125), groups=groups, device=0)
    names, ids, labels = gen._group_order(groups)
    assert len(names) == 7 and got.names == names and got.sizes.sum() == 140
    phi = gen.phi(ped, ids, device=0)
    ref = HO.hist(phi, got.edges, labels, 7)
    assert HO.same((got.counts, got.below, got.above), ref) and got.n_pairs == 140 * 139 // 2
    host = gen.phiHist(phi, bins=64, range=(0.0, 0.125), groups=groups, probandIDs=ids)
    assert HO.same((host.counts, host.below, host.above), ref) and host.names == names
    q = np.linspace(0.0, 1.0, 21)                                           # 21 quantiles: three device calls
    assert np.array_equal(gen.phiQuantile(ped, q, probandIDs=ids, device=0), HO.quantile(phi, q))


def test_row_shards_add_and_a_recomputed_result_is_counted_again(synth_case):
    _, _, pl, phi, _ = synth_case
    n = len(phi)
    edges = np.linspace(0.0, 2.0 ** -4, 65)
    labels, g, _ = _patterns(n)["interleaved"]
    full, full_g = _check(pl, phi, edges), _check(pl, phi, edges, labels, g)
    try:
        parts, parts_g = [], []
        for rows in ((0, 1111), (1111, n)):
            pl.compute_device(device=0, rows=rows)
            parts.append(_check(pl, phi[rows[0]:rows[1]], edges, row_begin=rows[0]))
            parts_g.append(_check(pl, phi[rows[0]:rows[1]], edges, labels, g, row_begin=rows[0]))
            assert pl.count_pairs() == HO.n_pairs(n, *rows)
            ranks = [0, pl.count_pairs() // 2, pl.count_pairs() - 1, 12345]
            _check_select(pl, phi[rows[0]:rows[1]], ranks, row_begin=rows[0])                 # over the shard's pairs only
        assert HO.same(tuple(x + y for x, y in zip(*parts)), full) and HO.same(tuple(x + y for x, y in zip(*parts_g)), full_g)
        for rows in ((n - 1, n), (0, 1), (2, 2)):                           # the last row has no pair; an empty shard
            pl.compute_device(device=0, rows=rows)
            c, b, a = _check(pl, phi[rows[0]:rows[1]], edges, row_begin=rows[0])
            assert c.sum() + b + a == (n - 1 if rows == (0, 1) else 0) == pl.count_pairs()
            _check(pl, phi[rows[0]:rows[1]], edges, labels, g, row_begin=rows[0])
            if rows == (0, 1):
                _check_select(pl, phi[:1], [0, n - 2, 7])
            else:
                with pytest.raises(ValueError):
                    pl.select([0])
    finally:
        pl.compute_device(device=0)                                          # (the module's plan holds the full result again)
    assert HO.same(_check(pl, phi, edges), full) and HO.same(_check(pl, phi, edges, labels, g), full_g)


def test_select(gen, synth_case, sorted_upper):
    ped, pro, pl, phi, distinct = synth_case
    small = gen.plan(ped, pro[:5])
    try:
        m = small.compute(device=0)
        _check_select(small, m, np.arange(10))                              # all 10 ranks of a 5-proband plan in one call
        _check_select(small, m, [9, 0, 9, 3, 3, 0])
    finally:
        small.close()
    rng = np.random.default_rng(16)
    ranks = rng.integers(0, N_PAIRS, 16)                                    # 16 ranks, unsorted
    assert np.array_equal(_check_select(pl, phi, ranks), sorted_upper[ranks])
    _check_select(pl, phi, [N_PAIRS - 1, 0, N_PAIRS - 1, 77, 77, N_PAIRS // 2])              # repeated and unsorted ranks
    zeros = int(np.count_nonzero(sorted_upper == 0))
    assert 2 < zeros < N_PAIRS
    got = _check_select(pl, phi, [0, zeros // 2, zeros - 1, zeros])         # inside the run of zeros and on both of its ends
    assert got[:3].tolist() == [0.0, 0.0, 0.0] and got[3] > 0
    top = _check_select(pl, phi, [N_PAIRS - 1])[0]
    assert top == pl.phi_over(float(distinct[0]))[2].max() == distinct[0]   # the maximum is phi_over's largest value
    _check_select(pl, phi, np.arange(40) * (N_PAIRS // 40))                 # 40 ranks: three device calls
    for bad in ([-1], [N_PAIRS], [0, N_PAIRS]):
        with pytest.raises(ValueError):
            pl.select(bad)
    q = [0.0, 0.5, 0.9, 0.99, 0.999, 1.0, 1 / 3, 0.123456789, 0.75]         # 9 quantiles: two device calls
    assert np.array_equal(gen.phiQuantile(ped, q, probandIDs=pro, device=0), HO.quantile(phi, q))


def test_consistency_with_count_over(synth_case):
    _, _, pl, phi, distinct = synth_case
    for t in (0.0, float(distinct[999]), float(np.nextafter(np.float64(distinct[999]), 1.0)), float(distinct[0])):
        c, b, a = pl.hist([t, math.inf])
        assert c[0] + a == pl.count_over(t) and b == N_PAIRS - pl.count_over(t)


def test_the_same_call_gives_the_same_bytes(synth_case):
    _, _, pl, phi, _ = synth_case
    labels, g, _ = _patterns(len(phi))["interleaved"]
    edges = np.linspace(0.0, 0.5, 4097)
    for call in (lambda: pl.hist(edges), lambda: pl.hist(edges[::64], labels, g), lambda: (pl.select([5, N_PAIRS // 2, N_PAIRS - 1]),)):
        x, y = call(), call()
        assert all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(x, y))


# ---- errors -----------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_plan_usable(gen):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(4000, 400, 10, skip_permille=50)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro)
    L, C = gen._capi.lib(), gen._capi
    dp = ctypes.POINTER(ctypes.c_double)
    edges = np.linspace(0.0, 2.0 ** -4, 33)
    labels = (np.arange(400) % 7).astype(np.int32)

    def c_hist(e):
        e = np.ascontiguousarray(e, dtype=np.float64)
        return L.genphi_result_hist(pl._h, len(e), e.ctypes.data_as(dp), 0, None, None, None, None, None)

    def c_select():
        r, v = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.float32)
        return L.genphi_result_select(pl._h, 1, r.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), v.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None)

    try:
        with pytest.raises(gen.GenphiDeviceError):                        # no resident result yet
            pl.hist(edges)
        with pytest.raises(gen.GenphiDeviceError):
            pl.select([0])
        assert c_hist(edges) == C.GENPHI_ERR_DEVICE and c_select() == C.GENPHI_ERR_DEVICE
        phi = pl.compute(device=0)
        t = float(np.unique(_upper(phi))[-20])
        counted = pl.count_over(t)                                        # the phiOver counts the library keeps ...
        assert counted == int(np.count_nonzero(_upper(phi).astype(np.float64) >= t))

        def good():
            _check(pl, phi, edges)
            _check(pl, phi, edges, labels, 7)
            _check_select(pl, phi, [0, 400 * 399 // 4, 400 * 399 // 2 - 1])
            assert np.array_equal(pl.result_to_host(), phi)
            r, c, v = pl.phi_over(t)                                      # ... still fit the result after every hist and select
            assert len(r) == counted and np.array_equal(v, phi[r, c]) and np.all(v.astype(np.float64) >= t) and pl.count_over(t) == counted

        good()
        with pytest.raises(ValueError):
            pl.hist([0.0, math.nan, 1.0])
        assert c_hist([0.0, math.nan, 1.0]) == C.GENPHI_ERR_ARG
        good()
        with pytest.raises(ValueError):
            pl.hist(edges, labels, 3)                                     # a label outside [-1, 3)
        with pytest.raises(ValueError):
            pl.select([400 * 399 // 2])
        good()
        pl.compute_device(device=0, storage64=True)                       # a Float64 result
        with pytest.raises(ValueError, match="Float32"):
            pl.hist(edges)
        with pytest.raises(ValueError, match="Float32"):
            pl.select([0])
        with pytest.raises(ValueError, match="Float32"):
            pl.count_pairs()
        assert c_hist(edges) == C.GENPHI_ERR_ARG and c_select() == C.GENPHI_ERR_ARG
        pl.compute_device(device=0)
        counted = pl.count_over(t)
        good()
        pl.release_device()
        with pytest.raises(gen.GenphiDeviceError):
            pl.hist(edges)
        with pytest.raises(gen.GenphiDeviceError):
            pl.select([0])
        assert c_hist(edges) == C.GENPHI_ERR_DEVICE and c_select() == C.GENPHI_ERR_DEVICE
        pl.compute_device(device=0)
        counted = pl.count_over(t)
        good()
    finally:
        pl.close()
