"""The GPU's Float64 sweep (GENPHI_FLAG_STORAGE_F64: level_full64_kernel, level_split64_kernel, level_naive64_kernel and the
sparse leading cuts; behind gen.f, the pairwise gen.phi, genphi_phi_pairs and compute_device(storage64=True)) against the
oracle's Float64 sweep (Pedigree.phi64 / phi_rows64), bit for bit wherever the result is a normal double, and against exact
kinships (tests/exact_kinship.py).  Deep inbred pedigrees throughout: there the kinships need more than 53 bits, so the
grouping of every Float64 sum shows in the last bits (a swapped pair of terms, a regrouped sum or a mixed-up rank word
changes them), which the shallow pedigrees of the older tests cannot show."""
import numpy as np
import pytest

from exact_kinship import ExactKinship, level_steps, max_rel_err, rel_err_bound

pytestmark = pytest.mark.gpu

TINY = np.finfo(np.float64).tiny
DENORM_MIN = 2.0 ** -1074


def _bits_equal(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got.view(np.uint64), want.view(np.uint64)):
        bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} entries differ; first {i}: {got[i]!r} vs {want[i]!r} "
                             f"({(got[i] - want[i]) / max(abs(want[i]), TINY):.2e} relative)")


def _ped(gen, ind, fa, mo, sort=True):
    return gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": np.ones(len(ind), dtype=np.int64)}, sort=sort)


def _sweep64(pl, **kw):
    pl.compute_device(storage64=True, **kw)
    return pl.result_to_host_f64().copy()


def _full_mantissas(m):
    """Entries whose last 8 mantissa bits are not all 0 (a shallow pedigree's dyadic kinships use a few leading bits only)."""
    return int(np.count_nonzero(np.asarray(m, dtype=np.float64).view(np.uint64) & np.uint64(0xFF)))


def _inexact(m, ex, pro):
    return int(np.count_nonzero(m != ex.float64(pro)))


def _deep_then_wide(n_gen, per_gen, layers, skip, seed=7):
    """deep_inbred(n_gen, per_gen) under `layers` generations of the given sizes: parents drawn from the generation above, or
    with probability `skip` from the one above that (members dragged along: the last cut in [dragged, new] order).
    Probands = the last layer."""
    from genlib_jl_amd import synth
    ind, fa, mo, _, last = synth.deep_inbred(n_gen, per_gen, 3)
    ind, fa, mo = list(ind), list(fa), list(mo)
    rng = np.random.default_rng(seed)
    prev2, prev, nxt = None, np.asarray(last), len(ind) + 1
    for size in layers:
        cur = np.arange(nxt, nxt + size)
        nxt += size
        for c in cur:
            sf = prev2 if prev2 is not None and rng.random() < skip else prev
            sm = prev2 if prev2 is not None and rng.random() < skip else prev
            ind.append(int(c)); fa.append(int(rng.choice(sf))); mo.append(int(rng.choice(sm)))
        prev2, prev = prev, cur
    a = lambda x: np.asarray(x, dtype=np.int64)
    return a(ind), a(fa), a(mo), a(prev)


def _f64_family(n_prev, cap_floats=None):
    """The Float64 kernel compute_f64 runs a dense step with n_prev source members on at kernel 0: 'full', 'split', 'naive'."""
    budget = 160 * 1024 if cap_floats is None else min(160 * 1024, 4 * cap_floats)
    r = (n_prev + 2) // 2 * 2
    return "full" if 16 * r <= budget else ("split" if 8 * r <= budget and n_prev < 65535 else "naive")


def test_deep_pedigree_float64_sweep_kernel0_and_kernel1(gen, oracle):
    """(a) 200 generations: kernel 0 (level_full64_kernel) and kernel 1 (level_naive64_kernel) equal the oracle's Float64
    sweep bit for bit; on a down-scaled twin the GPU stays within 2 L 2^-53 of the exact kinships while many of its entries
    are not the correctly rounded kinship (the test can tell groupings apart)."""
    from genlib_jl_amd import synth
    ind, fa, mo, _, pro = synth.deep_inbred(200, 50, 3)
    ped = _ped(gen, ind, fa, mo)
    want = oracle.Pedigree(ind, fa, mo).phi64(pro)
    pl = gen.plan(ped, pro)
    for kernel in (0, 1):
        _bits_equal(_sweep64(pl, kernel=kernel), want, f"deep_inbred(200, 50) kernel {kernel}")
    _bits_equal(_sweep64(pl, no_sparse=True), want, "deep_inbred(200, 50) no_sparse")
    pl.close()
    ind, fa, mo, _, pro = synth.deep_inbred(200, 10, 3)
    op = oracle.Pedigree(ind, fa, mo)
    ex = ExactKinship(ind, fa, mo)
    pl = gen.plan(_ped(gen, ind, fa, mo), pro)
    got = _sweep64(pl)
    pl.close()
    _bits_equal(got, op.phi64(pro), "deep_inbred(200, 10)")
    L = level_steps(op, pro)
    err = max_rel_err(got, ex.scaled(pro, pro), ex.S)
    print(f"deep_inbred(200, 10): GPU max relative error {err:.3e} = {err / 2.0 ** -53:.2f} x 2^-53, bound {rel_err_bound(L):.3e}")
    assert err <= rel_err_bound(L)
    assert _inexact(got, ex, pro) >= got.size // 5


def test_full64_block_sizes_and_column_chunks(gen, oracle):
    """(b) level_full64_kernel's block sizes (64: the deep upper levels; 256: 3,000 columns; 512 with two column chunks of
    512 x 20: 11,000 columns) on probands whose 60 parents have 120 generations of inbred ancestry.  Sampled rows (first,
    last, around 10,240) against phi_rows64, whole rows; kernel 1 on the same plan for the whole matrix."""
    from genlib_jl_amd import synth
    rng = np.random.default_rng(60)
    ind0, fa0, mo0, _, par = synth.deep_inbred(120, 60, 3)
    males, females = par[0::2], par[1::2]
    for n_pro in (3000, 11000):
        new = np.arange(len(ind0) + 1, len(ind0) + 1 + n_pro, dtype=np.int64)
        ind = np.concatenate([ind0, new])
        fa = np.concatenate([fa0, rng.choice(males, n_pro)])
        mo = np.concatenate([mo0, rng.choice(females, n_pro)])
        mo[len(ind0) + 5] = 0                                              # a one-parent proband
        ped = _ped(gen, ind, fa, mo)
        pl = gen.plan(ped, new)
        assert max(pl.levels()[0][:-1]) <= 60
        got = _sweep64(pl)
        assert got.shape == (n_pro, n_pro)
        rows = np.unique([0, 1, 5, 517, n_pro // 2, n_pro - 2, n_pro - 1] + ([10239, 10240, 10241] if n_pro > 10241 else []))
        want = oracle.Pedigree(ind, fa, mo).phi_rows64(new, rows)
        _bits_equal(got[rows], want, f"{n_pro} probands")
        _bits_equal(got[:, rows].T, want, f"{n_pro} probands, columns")
        assert _full_mantissas(want) > want.size // 4          # deep values: the last mantissa bits in use
        _bits_equal(_sweep64(pl, kernel=1), got, f"{n_pro} probands kernel 1")
        pl.close()


@pytest.mark.parametrize("family", ["split", "naive"])
def test_split64_and_naive64_at_kernel0(gen, oracle, family):
    """(c, d) level_split64_kernel and level_naive64_kernel at kernel 0: a small LDS budget (GENPHI_LDS_CAP_FLOATS) sends the
    small cuts of a deep pedigree through them; the whole matrix bit for bit against phi64, and row shards."""
    from genlib_jl_amd import synth
    ind, fa, mo, _, pro = synth.deep_inbred(200, 50, 3)
    ped = _ped(gen, ind, fa, mo)
    sizes = gen.plan(ped, pro).levels()[0]
    r_max = max((n + 2) // 2 * 2 for n in sizes[:-1])
    cap = 2 * r_max if family == "split" else 16
    fams = [_f64_family(n, cap) for n in sizes[:-1]]
    assert fams.count(family) >= len(fams) // 3, fams
    want = oracle.Pedigree(ind, fa, mo).phi64(pro)
    pl = gen.plan(ped, pro, tuning={"GENPHI_LDS_CAP_FLOATS": cap})
    _bits_equal(_sweep64(pl), want, f"{family}64, LDS cap {cap}")
    _bits_equal(_sweep64(pl, no_sparse=True), want, f"{family}64, LDS cap {cap}, no_sparse")
    parts = [_sweep64(pl, rows=r) for r in ((0, 1), (1, 31), (31, 49), (49, 50))]
    _bits_equal(np.concatenate(parts, axis=0), want, f"{family}64 row shards")
    pl.close()


def test_genea140_float64_whole_matrix(gen, oracle):
    """(c) genea140 in full: cuts of 10,240 to 13,654 members through level_split64_kernel, the rest through
    level_full64_kernel and the sparse leading cuts; with and without the sparse cuts, kernel 1, against phi64."""
    ped = gen.genealogy(gen.genea140)
    pro = gen.pro(ped)
    want = oracle.Pedigree.from_file(gen.genea140).phi64(pro)
    pl = gen.plan(ped, pro)
    sizes = pl.levels()[0]
    assert "split" in [_f64_family(n) for n in sizes[:-1]]
    _bits_equal(_sweep64(pl), want, "genea140")
    k, _ = pl.sparse_levels()
    assert k >= 2, k
    _bits_equal(_sweep64(pl, no_sparse=True), want, "genea140 no_sparse")
    _bits_equal(_sweep64(pl, kernel=1), want, "genea140 kernel 1")
    pl.close()


def test_wide_last_step_and_row_shards(gen, oracle):
    """(e) A WIDE last step (the last cut stored in [dragged, new] order, delivered through colmap) under 80 inbred
    generations, whole and in row shards of one row, the last row and a middle range."""
    ind, fa, mo, pro = _deep_then_wide(80, 40, [700, 900, 1200], 0.4)
    ped = _ped(gen, ind, fa, mo)
    n = len(pro)
    want = oracle.Pedigree(ind, fa, mo).phi64(pro)
    for cap in (400, 1024):
        pl = gen.plan(ped, pro, tuning={"GENPHI_LDS_CAP_FLOATS": cap, "GENPHI_NO_SMALL": 1})
        assert pl.step_modes()[-1] == 2, pl.step_modes()
        _bits_equal(_sweep64(pl), want, f"WIDE last step, cap {cap}")
        _bits_equal(_sweep64(pl, kernel=1), want, f"WIDE last step, cap {cap}, kernel 1")
        for r in ((0, 1), (n - 1, n), (300, 777)):
            _bits_equal(_sweep64(pl, rows=r), want[r[0]:r[1]], f"WIDE last step, cap {cap}, rows {r}")
        pl.close()
    pl = gen.plan(ped, pro)
    for r in ((0, 1), (n - 1, n), (300, 777)):
        _bits_equal(_sweep64(pl, rows=r), want[r[0]:r[1]], f"default plan, rows {r}")
    pl.close()


def test_float64_buffers_grow_and_are_released(gen, oracle):
    """The Float64 buffers of ONE plan over calls of different sizes and a release (the host contract test makes a single Float64 call):
    rows (3, 40), (0, 200), (5, 9), release_device(), (3, 40) again -- every result against the oracle's rows; the plan's device bytes
    never decrease while buffers are only grown, are 0 after the release, and a plan uploaded again holds what it held the first time."""
    from genlib_jl_amd import synth
    ind, fa, mo, _, pro = synth.random_mating(8000, 900, 9, skip_permille=40)
    ped = _ped(gen, ind, fa, mo)
    want = oracle.Pedigree(ind, fa, mo).phi_rows64(pro, np.arange(200))
    pl = gen.plan(ped, pro)
    held = []
    for r in ((3, 40), (0, 200), (5, 9)):
        _bits_equal(_sweep64(pl, rows=r), want[r[0]:r[1]], f"rows {r}")
        held.append(pl.device_bytes)
    assert 0 < held[0] <= held[1] <= held[2], held
    pl.release_device()
    assert pl.device_bytes == 0
    _bits_equal(_sweep64(pl, rows=(3, 40)), want[3:40], "rows (3, 40) after release_device")
    assert pl.device_bytes == held[0], (pl.device_bytes, held)
    pl.close()


def test_sparse_leading_cuts_float64(gen, oracle):
    """(f) The sparse leading cuts (csrc/sparse_levels.hip) writing the first dense Float64 matrix, against phi64, with and
    without them: a random pedigree whose calibration keeps at least two cuts as lists.  (genea140: above.)"""
    from genlib_jl_amd import synth
    ind, fa, mo, _, pro = synth.random_mating(30000, 3000, 10, skip_permille=0)
    ped = _ped(gen, ind, fa, mo)
    pl = gen.plan(ped, pro, tuning={"GENPHI_STAY_NARROW": 0})
    pl.compute()                                                          # calibration of the sparse cuts
    assert pl.sparse_levels()[0] >= 2, pl.sparse_levels()
    got = _sweep64(pl)
    _bits_equal(_sweep64(pl, no_sparse=True), got, "sparse vs no_sparse")
    rows = np.unique([0, 1, 1499, 2998, 2999] + list(np.random.default_rng(3).integers(0, 3000, 20)))
    _bits_equal(got[rows], oracle.Pedigree(ind, fa, mo).phi_rows64(pro, rows), "random_mating(30000, 3000, 10)")
    pl.close()


@pytest.mark.parametrize("shuffled", [False, True])
def test_pairwise_phi_and_phi_pairs_on_deep_pedigrees(gen, oracle, shuffled):
    """(g) gen.phi(ped[i], ped[j]) and genphi_phi_pairs on a 120-generation inbred pedigree: every value is the entry of
    phi64 over the named individuals (first occurrences, the sweep's proband list); with sort=False on a parents-first
    shuffle, where the file position is the rank that picks the grouping."""
    from genlib_jl_amd import synth, _capi
    ind, fa, mo, sex, _ = synth.deep_inbred(120, 30, 3)
    if shuffled:
        ind, fa, mo, sex = synth.parents_first_shuffle(ind, fa, mo, sex, seed=3)
    ped = _ped(gen, ind, fa, mo, sort=not shuffled)
    op = oracle.Pedigree(ind, fa, mo, sort=not shuffled)
    rng = np.random.default_rng(12)
    a = rng.choice(ind[len(ind) // 2:], 40)
    b = rng.choice(ind[len(ind) // 2:], 40)
    a[3] = b[3]                                                           # a self pair
    named = np.array(list(dict.fromkeys(int(x) for pair in zip(a, b) for x in pair)), dtype=np.int64)
    m = op.phi64(named)
    at = {int(x): k for k, x in enumerate(named)}
    want = np.array([m[at[int(x)], at[int(y)]] for x, y in zip(a, b)])
    got = _capi.phi_pairs(ped.ind, ped.father, ped.mother, a, b)
    _bits_equal(got, want, "phi_pairs")
    assert _full_mantissas(want) > len(want) // 4
    for x, y in list(zip(a, b))[:4]:
        one = op.phi64([int(x), int(y)])
        assert gen.phi(ped[int(x)], ped[int(y)]) == one[0, 1 if x != y else 0], (x, y)


def test_inbreeding_f_on_a_deep_pedigree(gen, oracle):
    """(h) gen.f of every individual of a 150-generation inbred pedigree with one-parent and selfed members: each value is
    Float32(phi64[father, mother]) over the sorted parents bit for bit, and within 1 Float32 ulp of Float32(exact)."""
    from genlib_jl_amd import synth
    ind, fa, mo, _, _ = synth.deep_inbred(150, 14, 3)
    mo = mo.copy()
    mo[100::97] = 0                                                       # one-parent members
    self_ = np.arange(60, len(ind), 131)
    mo[self_] = fa[self_]                                                 # selfed members: father == mother
    ped = _ped(gen, ind, fa, mo)
    got = gen.f(ped, ind)
    assert got.dtype == np.float32
    both = (fa != 0) & (mo != 0)
    parents = np.unique(np.concatenate([fa[both], mo[both]]))
    m = oracle.Pedigree(ind, fa, mo).phi64(parents)
    want = np.zeros(len(ind), dtype=np.float32)
    want[both] = m[np.searchsorted(parents, fa[both]), np.searchsorted(parents, mo[both])].astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.flatnonzero(got != want)[:5]
    assert np.all(got[~both] == 0) and np.all(got[self_] >= 0.5)
    ex = ExactKinship(ind, fa, mo)
    exact32 = np.zeros(len(ind), dtype=np.float32)
    exact32[both] = ex.pairs64(fa[both], mo[both]).astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(exact32), np.finfo(np.float32).tiny)).astype(np.float32)
    diff = np.abs(got.astype(np.float64) - exact32.astype(np.float64))
    print(f"gen.f on deep_inbred(150, 14): {int(np.count_nonzero(got != exact32))} of {len(got)} differ from Float32(exact)")
    assert np.all(diff <= ulp), np.flatnonzero(diff > ulp)[:5]


@pytest.mark.parametrize("depth", [505, 511, 512, 520, 536, 537, 540])
def test_float64_subnormal_kinships(gen, oracle, depth):
    """(i) Kinships 2^-(2 depth) of two single-parent lines: normal down to 2^-1022, subnormal to 2^-1074, then 0 -- the
    exact values (powers of two), no flush to zero, through a plan and through the pairwise gen.phi."""
    from genlib_jl_amd import synth
    ind, fa, mo, _, pro = synth.chain_two_lines(depth)
    ped = _ped(gen, ind, fa, mo)
    want = ExactKinship(ind, fa, mo).float64(pro)
    assert want[0, 1] == np.ldexp(1.0, -2 * depth)
    pl = gen.plan(ped, pro)
    for kernel in (0, 1):
        _bits_equal(_sweep64(pl, kernel=kernel), want, f"chain_two_lines({depth}) kernel {kernel}")
    pl.close()
    assert gen.phi(ped[int(pro[0])], ped[int(pro[1])]) == want[0, 1]


def test_float64_subnormal_inexact_kinships(gen, oracle):
    """(i) Inexact kinships sinking through the subnormal range: two single-parent lines of 545 generations below two
    members of a 60-generation inbred line, their members at several depths as probands.  Where phi64 is normal the GPU
    equals it bit for bit; below 2^-1022 the GPU sums then scales once where the recursion halves each term, so it is held
    to |gpu - exact| <= 4 x 2^-1074 there."""
    from genlib_jl_amd import synth
    ind, fa, mo, _, last = synth.deep_inbred(60, 12, 3)
    ind, fa, mo = list(ind), list(fa), list(mo)
    nxt, tips = len(ind) + 1, []
    for top in (last[0], last[3]):
        line, parent = [], int(top)
        for _ in range(545):
            ind.append(nxt); fa.append(parent); mo.append(0)
            line.append(nxt); parent = nxt; nxt += 1
        tips.append(line)
    ind, fa, mo = (np.asarray(x, dtype=np.int64) for x in (ind, fa, mo))
    depths = [500, 505, 510, 511, 512, 513, 515, 520, 525, 530, 535, 536, 537, 538, 544]
    pro = np.array([tips[0][d] for d in depths] + [tips[1][d] for d in depths], dtype=np.int64)
    ped = _ped(gen, ind, fa, mo)
    ex = ExactKinship(ind, fa, mo)
    exact = ex.float64(pro)
    m64 = oracle.Pedigree(ind, fa, mo).phi64(pro)
    pl = gen.plan(ped, pro)
    for kernel in (0, 1):
        got = _sweep64(pl, kernel=kernel)
        normal = m64 >= TINY
        _bits_equal(got[normal], m64[normal], f"normal entries, kernel {kernel}")
        sub = ~normal
        assert np.count_nonzero(sub & (exact > 0)) >= 20
        err = np.abs(got[sub] - exact[sub])
        print(f"kernel {kernel}: {int(np.count_nonzero(sub))} entries below 2^-1022, max |gpu - exact| = {err.max() / DENORM_MIN:.0f} x 2^-1074")
        assert np.all(err <= 4 * DENORM_MIN)
        assert np.all(got[sub & (exact >= 8 * DENORM_MIN)] > 0)           # no flush to zero
    pl.close()
