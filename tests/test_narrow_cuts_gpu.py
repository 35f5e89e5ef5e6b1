"""The early dense cuts of a Float32 sweep kept as 16- and 24-bit integers (csrc/cut_format.h): every entry of cut c is a multiple of
2^-(2c+1) (csrc/sparse_levels.h, "Exactness"), so cuts up to 7 / up to 11 lose nothing when the sparse -> dense step and the certified-rows
SPLIT kernel write them as integers of that unit and the SPLIT kernel decodes them where it stages a row.  Every case is compared, ==, with the oracle and
with the same plan under GENPHI_NO_NARROW=1 (every cut Float32); the formats a sweep used and its encode guard are read back through
genphi_plan_cut_formats, so that a case that silently stayed Float32 fails."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# every level SPLIT on the certified-rows kernel (no FULL kernel, no fused small levels, no in-place runs), list cuts whatever their width
SPLIT = {"FULL_MAX_FLOATS": 0, "NO_SMALL": 1, "NO_STAY": 1, "SPARSE_MIN_CUT": 0}
F32, U16, U24 = 0, 1, 2


def _layered(sizes, seed, p_one_parent=0.0, p_skip=0.0):
    """Discrete generations of the given sizes, every member of a generation a parent of the next (so cut c is generation c when
    p_skip = 0); p_one_parent: share of members with one parent unknown; p_skip: share of parents drawn two generations up (members
    dragged along a cut).  Probands = the last generation."""
    rng = np.random.default_rng(seed)
    ind, fa, mo, sex, gens = [], [], [], [], []
    nxt = 1
    for g, n in enumerate(sizes):
        ids = np.arange(nxt, nxt + n, dtype=np.int64)
        nxt += n
        s = (np.arange(n) % 2 + 1).astype(np.int64)
        f = np.zeros(n, dtype=np.int64)
        m = np.zeros(n, dtype=np.int64)
        if g > 0:
            males, females = gens[g - 1][0::2], gens[g - 1][1::2]
            f = np.where(np.arange(n) < len(males), rng.permutation(males)[np.arange(n) % len(males)], rng.choice(males, n))
            m = np.where(np.arange(n) < len(females), rng.permutation(females)[np.arange(n) % len(females)], rng.choice(females, n))
            if g > 1 and p_skip > 0:
                up = rng.random(n) < p_skip
                f = np.where(up, rng.choice(gens[g - 2][0::2], n), f)
                up = rng.random(n) < p_skip
                m = np.where(up, rng.choice(gens[g - 2][1::2], n), m)
            u = rng.random(n)
            f = np.where(u < p_one_parent / 2, 0, f)
            m = np.where((u >= p_one_parent / 2) & (u < p_one_parent), 0, m)
        ind.append(ids); fa.append(f); mo.append(m); sex.append(s); gens.append(ids)
    cat = lambda v: np.concatenate(v).astype(np.int64)      # noqa: E731
    return cat(ind), cat(fa), cat(mo), cat(sex), gens[-1].copy()


def _expected_formats(k, n_cuts):
    """The rule of cut_format.h for a sweep whose steps above the list cuts are all certified-rows SPLIT steps: the sparse -> dense step
    (step k) starts the narrow run at cut k + 1, 16 bits through cut 7, 24 bits through cut 11, and the cut the proband step reads is
    Float32 like its own."""
    return [(U16 if c <= 7 else U24) if (k >= 1 and k + 1 <= c <= 11 and c < n_cuts - 2) else F32 for c in range(n_cuts)]


def _sweeps(gen, ped, pro, want, tuning, k_forced=None, rows=None, replays=0):
    """One plan with the narrow cuts and one without; both == want.  Returns the formats of the narrow plan."""
    out = None
    for no_narrow in (0, 1):
        t = dict(SPLIT, **tuning, NO_NARROW=no_narrow)
        if k_forced is not None:
            t["SPARSE_K"] = k_forced
        pl = gen.plan(ped, pro, tuning=t)
        got = pl.compute()
        assert got.dtype == np.float32 and np.array_equal(got, want), (tuning, no_narrow, int((got != want).sum()))
        fmt, guard = pl.cut_formats()
        k = pl.sparse_levels()[0]
        assert guard == 0 and len(fmt) == len(pl.levels()[0])
        assert fmt == ([F32] * len(fmt) if no_narrow else _expected_formats(k, len(fmt))), (fmt, k, no_narrow)
        if k_forced is not None:
            assert k == k_forced
        if rows is not None:
            for a, b in rows:
                assert np.array_equal(pl.compute(rows=(a, b)), want[a:b]), (a, b, no_narrow)
                assert pl.cut_formats() == (fmt, 0)
        for _ in range(replays):                                  # no timing: the second call on replays the captured graph
            pl.compute_device()
            assert pl.cut_formats() == (fmt, 0)
        if replays:
            assert np.array_equal(pl.result_to_host(), want)
        if not no_narrow:
            out = fmt
        pl.close()
    return out


def test_every_format_pair_in_one_sweep(gen, oracle):
    """16 cuts deep: the sparse -> dense writer, u16 -> u16, u16 -> u24, u24 -> u24 and u24 -> f32 steps in one sweep; with the last list
    cut by calibration and forced to 3 (the first dense cut, 4, then starts the narrow run) and to 8 (cut 9 is written in 24 bits by the
    sparse -> dense step), and a proband step close enough to end the run early (u16 -> f32)."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(9600, 600, 16, skip_permille=0)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    want = oracle.Pedigree(ind, fa, mo).phi(pro)
    fmt = _sweeps(gen, ped, pro, want, {}, k_forced=3)
    assert fmt[3:13] == [F32] + [U16] * 4 + [U24] * 4 + [F32]
    _sweeps(gen, ped, pro, want, {})                                  # last list cut by calibration: the formats follow from it
    fmt = _sweeps(gen, ped, pro, want, {}, k_forced=8)
    assert fmt[8:13] == [F32] + [U24] * 3 + [F32]
    ind, fa, mo, sex, pro = synth.random_mating(4800, 600, 8, skip_permille=0)                 # 8 cuts: cut 5 is the last one a non-proband step reads
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    fmt = _sweeps(gen, ped, pro, oracle.Pedigree(ind, fa, mo).phi(pro), {}, k_forced=3)
    assert fmt == [F32] * 4 + [U16] * 2 + [F32] * 2


@pytest.fixture(scope="module")
def corner_case(oracle):
    # cuts 4 .. 8 (16 bits, the last one 24) and 8 .. 12 (24 bits, the last one Float32) with 0, 1, 5, 15, 0 members beyond a multiple of
    # 16: n_prev and n of the steps that read narrow cuts take every remainder in both formats; wider than one column chunk of
    # GENPHI_MAX_CPT = 4 (4096 columns), the last chunk ragged
    sizes = [4100, 4100, 4100, 4100, 4112, 4113, 4117, 4127, 4128, 4129, 4133, 4143, 4144, 4100, 4100]
    ind, fa, mo, sex, pro = _layered(sizes, seed=5)
    return sizes, (ind, fa, mo, sex, pro), oracle.Pedigree(ind, fa, mo).phi(pro)


@pytest.mark.parametrize("nt", [1024, 512])
def test_widths_at_the_packing_corners_in_two_chunks(gen, corner_case, nt):
    sizes, (ind, fa, mo, sex, pro), want = corner_case
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    pl = gen.plan(ped, pro, tuning=SPLIT)
    assert pl.levels()[0] == sizes
    pl.close()
    fmt = _sweeps(gen, ped, pro, want, {"MAX_CPT": 4, "FAST_NT": nt}, k_forced=3)
    assert fmt[4:13] == [U16] * 4 + [U24] * 4 + [F32]


def test_dragged_and_one_parent_rows_diagonal_and_none_row(gen, oracle):
    """Overlapping generations and unknown parents: rows finished from the hub's expansion alone (dragged and one-parent members), the
    diagonal patch of new members and gathers from the all-zero "none" row, all on narrow cuts."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(6000, 400, 12, skip_permille=150)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    fmt = _sweeps(gen, ped, pro, oracle.Pedigree(ind, fa, mo).phi(pro), {}, k_forced=3)
    assert fmt[4:10] == [U16] * 4 + [U24] * 2
    ind, fa, mo, sex, pro = _layered([700, 650, 720, 690, 705, 713, 641, 699, 702, 655, 671, 708, 500], seed=9, p_one_parent=0.2, p_skip=0.15)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    for k in (2, 3):
        fmt = _sweeps(gen, ped, pro, oracle.Pedigree(ind, fa, mo).phi(pro), {"MAX_GROUP": 3}, k_forced=k)
        assert fmt[k + 1:11] == [U16] * (7 - k) + [U24] * 3


def test_deep_inbreeding_fills_the_range(gen, oracle):
    """Three sires per generation: kinships and diagonals climb towards 1, the top of a cut's integer range (cut 7: 2^15 - 1, cut 11:
    2^23 - 1 at most)."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.deep_inbred(16, 500, 3)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    want = oracle.Pedigree(ind, fa, mo).phi(pro)
    assert want.max() > 0.6
    for k in (1, 3):
        fmt = _sweeps(gen, ped, pro, want, {}, k_forced=k)
        assert fmt[k + 1:13] == [U16] * (7 - k) + [U24] * 4 + [F32]


def test_row_shards_and_graph_replay(gen, oracle):
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(7200, 600, 12, skip_permille=20)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    want = oracle.Pedigree(ind, fa, mo).phi(pro)
    fmt = _sweeps(gen, ped, pro, want, {}, k_forced=3, rows=[(0, 200), (200, 201), (201, 600)], replays=3)
    assert fmt[4:10] == [U16] * 4 + [U24] * 2
