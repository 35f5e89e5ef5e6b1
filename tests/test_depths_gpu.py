"""gen.depths on the GPU (csrc/depth.hip) against the oracles of tests/depths_oracle.py.  Every comparison is exact; equal_nan applies
to `mean` only."""
import numpy as np
import pytest

import depths_oracle as DO
from random_pedigree import random_pedigree
from test_depth_host import skipping_ladder
from test_occ_reference import QUIRK_ANC, QUIRK_PRO, doubling_chain, quirk_pedigree

pytestmark = pytest.mark.gpu

GROUP_ROWS = 16            # kDepthGroupRows of csrc/depth.hip: the last-list items one row group of the by = ancestor reduction folds


def _args(ped):
    return ped.ind, ped.father, ped.mother


def compute(gen, args, pro, anc, by="pair", panel_cols=0, panels_per_launch=0, twice=False):
    """((min, max, paths, mean), stats) of one handle; twice: computed again on the same handle, which must give the same bytes."""
    h = gen.DepthPlan(*args, pro, anc, by=by, panel_cols=panel_cols, panels_per_launch=panels_per_launch)
    try:
        h.compute()
        out = h.result_to_host()
        if twice:
            h.compute()
            again = h.result_to_host()
            assert [a.tobytes() for a in again] == [a.tobytes() for a in out]
        return out, h.stats()
    finally:
        h.close()


def same(got, want, cols=None):
    """got: (min, max, paths, mean) of the library; want: a Depths of the oracle (cols: its first columns only)."""
    lo, hi, paths, mean = got
    pick = (lambda a: a) if cols is None else (lambda a: a[:, :cols])
    assert lo.dtype == hi.dtype == np.int16 and paths.dtype == np.int64 and mean.dtype == np.float64
    assert np.array_equal(paths, pick(want.paths)), np.argwhere(paths != pick(want.paths))[:5]
    assert np.array_equal(lo, pick(want.min)), np.argwhere(lo != pick(want.min))[:5]
    assert np.array_equal(hi, pick(want.max)), np.argwhere(hi != pick(want.max))[:5]
    assert np.array_equal(mean, pick(want.mean), equal_nan=True)


@pytest.mark.parametrize("name", ["geneaJi", "genea140"])
def test_bundled_pedigrees_against_the_oracle_and_two_other_kernels(gen, name):
    """All probands x all founders; `min` also against gen.meioses (csrc/dist.hip) and `paths` against gen.occ (csrc/occ.hip)."""
    ped = gen.genealogy(getattr(gen, name))
    pro, anc = gen.pro(ped), gen.founder(ped)
    want = DO.depths_exact(*_args(ped), pro, anc)
    d = gen.depths(ped)
    assert d.by == "pair" and np.array_equal(d.pro, pro) and np.array_equal(d.ancestors, anc)
    same((d.min, d.max, d.paths, d.mean), want)
    assert np.array_equal(d.min, gen.meioses(ped))
    assert np.array_equal(d.paths, gen.occ(ped).T)
    if name == "genea140":
        assert (int(d.max.max()), int(d.paths.max())) == (17, 176)
    for by in ("proband", "ancestor"):
        r = gen.depths(ped, by=by)
        same((r.min, r.max, r.paths, r.mean), DO.reduce_depths(want, by))
    if name == "genea140":
        # one panel of all 7,399 columns: 29 chunks of 256 columns, more than the by = ancestor reduction deals to blocks (16)
        got, st = compute(gen, _args(ped), pro, anc, by="ancestor", panel_cols=len(anc))
        assert st["panel_cols"] == 7399
        same(got, DO.reduce_depths(want, "ancestor"))


@pytest.fixture(scope="module")
def mixed():
    """About 400 individuals with overlapping generations, one-parent members and founders anywhere; 70 probands (leaves, members with
    children, repeats) x 300 distinct ancestors (founders, members with parents, probands, unrelated members)."""
    rng = np.random.default_rng(4711)
    ind, fa, mo, _ = random_pedigree(rng, 400, p_founder=0.08, p_one_parent=0.15, p_selfing=0.02, max_back=45, max_depth=30)
    pro = rng.choice(ind, size=64, replace=False)
    pro = np.concatenate([pro, pro[:6]]).astype(np.int64)
    anc = rng.permutation(ind)[:300].astype(np.int64)
    want = DO.depths_exact(ind, fa, mo, pro, anc)
    assert np.isin(pro, anc).any() and np.isin(pro, np.union1d(fa, mo)).any() and (want.paths == 0).any() and int(want.paths.max()) > 100
    assert ((fa == 0) != (mo == 0)).any()
    return (ind, fa, mo), pro, anc, want


@pytest.mark.parametrize("n_anc", [1, 2, 3, 5, 9, 17, 33, 64, 65, 257, 300])
def test_every_lanes_per_row_form_and_the_loop_tail(gen, mixed, n_anc):
    """One panel of n_anc columns: 1, 2, 4, 8, 16, 32 and 64 lanes per row; 65: a second access of a lane; 257 and 300: a second turn of the
    loop of four accesses."""
    args, pro, anc, want = mixed
    got, st = compute(gen, args, pro, anc[:n_anc])
    assert st["panel_cols"] == n_anc and st["launches"] > 0 and st["algorithmic_bytes"] >= 20 * len(pro) * n_anc
    same(got, want, cols=n_anc)


@pytest.mark.parametrize("per_launch", [1, 3, 0])
@pytest.mark.parametrize("width", [1, 7, 8, 64, 100])
def test_forced_panels(gen, mixed, width, per_launch):
    """300 ancestors in panels of 1, 7 (ragged last panel of 6), 8, 64 (the last of 44) and 100 columns; one, three and all panels per launch."""
    args, pro, anc, want = mixed
    for by in ("pair", "proband", "ancestor"):
        got, st = compute(gen, args, pro, anc, by=by, panel_cols=width, panels_per_launch=per_launch)
        assert st["panel_cols"] == width
        same(got, want if by == "pair" else DO.reduce_depths(want, by))


def test_hand_made_pedigree(gen):
    """quirk_pedigree (tests/test_occ_reference.py) with QUIRK_PRO = [12, 8, 3, 12, 10, 1] x QUIRK_ANC = [1, 1, 3, 8, 10, 5, 11, 4]: 8 and 3
    are dragged into the last cut (copy items); 8, 10 and 1 are listed ancestors (0, 0, 1, 0.0); 11 is unrelated (-1, -1, 0, NaN); 4 and
    9 have one parent; 12 is listed twice; 1 is listed twice (equal columns)."""
    ped = quirk_pedigree(gen)
    want = DO.depths_literal(*_args(ped), QUIRK_PRO, QUIRK_ANC)
    d = gen.depths(ped, QUIRK_PRO, QUIRK_ANC)
    same((d.min, d.max, d.paths, d.mean), want)
    assert (d.min[0, 0], d.max[0, 0], d.paths[0, 0], d.mean[0, 0]) == (3, 4, 4, 15 / 4)                 # 12 -> 1
    for i, j in ((1, 3), (4, 4), (5, 0)):                                                               # 8, 10 and 1 to themselves
        assert (d.min[i, j], d.max[i, j], d.paths[i, j], d.mean[i, j]) == (0, 0, 1, 0.0)
    assert (d.min[:, 6] == -1).all() and (d.max[:, 6] == -1).all() and (d.paths[:, 6] == 0).all() and np.isnan(d.mean[:, 6]).all()
    assert np.array_equal(d.paths[:, 0], d.paths[:, 1]) and np.array_equal(d.mean[:, 0], d.mean[:, 1], equal_nan=True)
    assert np.array_equal(d.paths[0], d.paths[3]) and np.array_equal(d.max[0], d.max[3])
    r = gen.depths(ped, QUIRK_PRO, QUIRK_ANC, by="ancestor")                                            # duplicated ancestors: equal entries
    same((r.min, r.max, r.paths, r.mean), DO.reduce_depths(want, "ancestor"))
    distinct = [1, 3, 8, 10, 5, 11, 4]
    r = gen.depths(ped, QUIRK_PRO, distinct, by="proband")
    same((r.min, r.max, r.paths, r.mean), DO.reduce_depths(DO.depths_literal(*_args(ped), QUIRK_PRO, distinct), "proband"))
    with pytest.raises(ValueError, match="twice"):
        gen.depths(ped, QUIRK_PRO, QUIRK_ANC, by="proband")


@pytest.mark.parametrize("panel", [0, 16])
@pytest.mark.parametrize("n_rows", [1, GROUP_ROWS - 1, GROUP_ROWS, GROUP_ROWS + 1, 63, 64, 65, 129, 16 * GROUP_ROWS + 1])
def test_by_ancestor_at_the_row_group_edges(gen, mixed, n_rows, panel):
    """The by = ancestor reduction folds GROUP_ROWS = 16 items of the last list per row group: a last list of exactly 1, 15, 16, 17, then
    63, 64, 65 and 129 items (a short last group, whole groups, one item over; 64 and 65 also end and begin a block of four row groups at
    64 lanes per row) and 257 (one item over a block of 16 row groups at panels of 16 columns).  The ancestors include every founder, so
    every proband has a row; the probands are leaves, so none waits in a slot: the last list holds one item per listed proband."""
    (ind, fa, mo), _, anc, _ = mixed
    founders = ind[(fa == 0) & (mo == 0)]
    anc = np.union1d(founders, anc[:120])
    leaves = np.setdiff1d(np.setdiff1d(ind, np.union1d(fa, mo)), founders)
    assert len(leaves) > 20
    pro = np.resize(leaves, n_rows).astype(np.int64)
    want = DO.reduce_depths(DO.depths_exact(ind, fa, mo, pro, anc), "ancestor")
    assert int(want.paths.sum()) > n_rows
    got, _ = compute(gen, (ind, fa, mo), pro, anc, by="ancestor", panel_cols=panel, twice=True)
    same(got, want)


@pytest.mark.parametrize("per_launch", [0, 2])
def test_by_proband_across_panels_of_seven(gen, mixed, per_launch):
    args, pro, anc, want = mixed
    got, st = compute(gen, args, pro, anc, by="proband", panel_cols=7, panels_per_launch=per_launch, twice=True)
    assert st["panel_cols"] == 7
    same(got, DO.reduce_depths(want, "proband"))
    # the default panel (one panel of 300 columns, 64 lanes per row) gives the same bytes
    one, _ = compute(gen, args, pro, anc, by="proband")
    assert [a.tobytes() for a in one] == [a.tobytes() for a in got]


def test_genlib_wrappers_on_geneaJi(gen):
    ped = gen.genealogy(gen.geneaJi)
    ids = np.array([1, 2, 29, 17, 2], dtype=np.int64)                     # 17: a founder (0, 0, 0.0)
    want = DO.reduce_depths(DO.depths_literal(*_args(ped), ids, gen.founder(ped)), "proband")
    lo, hi, mean = gen.genMin(ped, ids), gen.genMax(ped, ids), gen.genMean(ped, ids)
    assert (lo.dtype, hi.dtype, mean.dtype) == (np.int16, np.int16, np.float64)
    assert np.array_equal(lo, want.min) and np.array_equal(hi, want.max) and np.array_equal(mean, want.mean)
    assert (lo[3], hi[3], mean[3]) == (0, 0, 0.0) and lo[1] == lo[4] and mean[1] == mean[4]
    assert np.array_equal(gen.genMax(ped), DO.reduce_depths(DO.depths_exact(*_args(ped), gen.pro(ped), gen.founder(ped)), "proband").max)


@pytest.mark.parametrize("skip", [False, True])
def test_ladders_of_47_steps(gen, skip):
    """The sib-mating ladder (96 individuals): 2^46 paths of 47 meioses from the last members to either founder, the packed fields at their
    limit; with one generation-skipping mate min 46 < mean 140 / 3 < max 47."""
    ind, fa, mo = skipping_ladder() if skip else doubling_chain(48)
    pro, anc = [96, 95, 96, 92, 1], [1, 2, 93, 96, 50]
    want = DO.depths_exact(ind, fa, mo, pro, anc)
    got, _ = compute(gen, (ind, fa, mo), pro, anc, twice=True)
    same(got, want)
    lo, hi, paths, mean = got
    if skip:
        assert (lo[0, 0], hi[0, 0], paths[0, 0], mean[0, 0]) == (46, 47, 3 * 2 ** 44, 140 / 3)
    else:
        assert (lo[0, 0], hi[0, 0], paths[0, 0], mean[0, 0]) == (47, 47, 2 ** 46, 47.0)
    assert paths[1, 1] == 2 ** 46
    for by in ("proband", "ancestor"):
        got, _ = compute(gen, (ind, fa, mo), pro, anc, by=by, panel_cols=2, twice=True)
        same(got, DO.reduce_depths(want, by))


def test_repeatable_and_empty(gen, mixed):
    args, pro, anc, want = mixed
    for by in ("pair", "proband", "ancestor"):
        got, _ = compute(gen, args, pro, anc, by=by, panel_cols=24, panels_per_launch=5, twice=True)
        same(got, want if by == "pair" else DO.reduce_depths(want, by))
    # the default rule: one panel of 300 columns, whose second chunk of 256 columns is ragged (by = ancestor: another block)
    for by in ("proband", "ancestor"):
        got, st = compute(gen, args, pro, anc, by=by, twice=True)
        assert st["panel_cols"] == 300
        same(got, DO.reduce_depths(want, by))
    ped = gen.genealogy(gen.geneaJi)
    for pro, anc in (([], [17, 19]), ([1, 2], []), ([], [])):
        for by, shape in (("pair", (len(pro), len(anc))), ("proband", (len(pro),)), ("ancestor", (len(anc),))):
            got, st = compute(gen, _args(ped), pro, anc, by=by, twice=True)
            assert all(a.shape == shape for a in got) and st["launches"] == 0
            assert (got[0] == -1).all() and (got[1] == -1).all() and (got[2] == 0).all() and np.isnan(got[3]).all()


def test_result_device_pointers_and_pitch(gen, mixed):
    """The resident result: four arrays at a common row pitch of n_anc rounded up to 8 entries, read back with plain device copies."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    args, pro, anc, want = mixed
    n_anc = 13
    h = gen.DepthPlan(*args, pro, anc[:n_anc])
    try:
        with pytest.raises(ValueError, match="nothing computed"):
            h.result_device()
        h.compute()
        d = h.result_device()
        assert d["ld"] == 16 and all(d[k] for k in ("min", "max", "paths", "mean"))
        for name, dtype in (("min", np.int16), ("max", np.int16), ("paths", np.int64), ("mean", np.float64)):
            buf = np.empty((len(pro), d["ld"]), dtype=dtype)
            assert hip.hipMemcpy(ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(d[name]), ctypes.c_size_t(buf.nbytes), 2) == 0      # device to host
            assert np.array_equal(buf[:, :n_anc], getattr(want, name)[:, :n_anc], equal_nan=name == "mean"), name
    finally:
        h.close()
    for by, n in (("proband", len(pro)), ("ancestor", n_anc)):
        h = gen.DepthPlan(*args, pro, anc[:n_anc], by=by)
        try:
            h.compute()
            d = h.result_device()
            buf = np.empty(n, dtype=np.int64)
            assert hip.hipMemcpy(ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(d["paths"]), ctypes.c_size_t(buf.nbytes), 2) == 0
            assert d["ld"] == (1 if by == "proband" else n_anc) and np.array_equal(buf, h.result_to_host()[2])
        finally:
            h.close()
