"""gen.depths on 60 random cases drawn with the generator of tests/random_pedigree.py: the three modes, random forced panel widths and
panels per launch, against depths_exact of tests/depths_oracle.py with no tolerance.  A drawn case is skipped only where its schedule
exceeds the 47 steps the packed counts hold; at most 5 % of the cases may be."""
import numpy as np
import pytest

import depths_oracle as DO
from random_pedigree import random_pedigree

N_CASES = 60
SEED = 20261019
MAX_SKIPPED = N_CASES * 5 // 100


def draw(case):
    """(ind, father, mother), probands, ancestors, by, panel_cols, panels_per_launch of one case."""
    rng = np.random.default_rng(SEED * 1000 + case)
    n = int(rng.integers(2, 320))
    p_founder = float(rng.choice([0.03, 0.1, 0.3]))
    p_one = float(rng.choice([0.0, 0.1, 0.4]))
    p_self = float(rng.choice([0.0, 0.05]))
    max_back = int(rng.choice([3, 10, 40, 150]))
    # 48 generations: exactly the 47 steps the packed counts hold; None: as deep as the draws make it (may exceed them)
    max_depth = [None, 12, 20, 30, 40, 48, 48, 48][int(rng.integers(0, 8))]
    ind, fa, mo, _ = random_pedigree(rng, n, p_founder, p_one, p_self, max_back, max_depth)
    by = ("pair", "proband", "ancestor")[case % 3]
    pro = rng.integers(1, n + 1, size=int(rng.integers(1, 90))).astype(np.int64)                # members of any depth, repeats
    kind = int(rng.integers(0, 3))
    if kind == 0:
        anc = ind[(fa == 0) & (mo == 0)]
    elif kind == 1:
        anc = rng.permutation(ind)[:int(rng.integers(1, n + 1))]
    else:
        anc = np.concatenate([rng.integers(1, n + 1, size=int(rng.integers(1, 150))), pro[:2]])   # repeats, probands
    anc = anc.astype(np.int64)
    if by == "proband":
        anc = anc[np.sort(np.unique(anc, return_index=True)[1])]                                 # no ancestor twice, the drawn order
    panel_cols = int(rng.choice([0, 0, 1, 2, 3, 5, 8, 13, 16, 33, 64, 70]))
    per_launch = int(rng.choice([0, 0, 1, 2, 5]))
    return (ind, fa, mo), pro, anc, by, panel_cols, per_launch


def plan(gen, case):
    """The case and its handle, or None where the schedule exceeds 47 steps (the only reason to skip a case)."""
    args, pro, anc, by, panel_cols, per_launch = draw(case)
    try:
        h = gen.DepthPlan(*args, pro, anc, by=by, panel_cols=panel_cols, panels_per_launch=per_launch)
    except ValueError as e:
        assert "at most 47 steps" in str(e), e
        return (args, pro, anc, by), None
    return (args, pro, anc, by), h


def test_the_drawn_cases_plan_within_the_bound(gen):
    """Planning needs no device: at most 5 % of the 60 cases exceed 47 steps, all three modes and forced panels are drawn."""
    skipped, modes, forced = 0, set(), 0
    for case in range(N_CASES):
        (_, _, _, by), h = plan(gen, case)
        if h is None:
            skipped += 1
            continue
        h.close()
        modes.add(by)
        forced += draw(case)[4] > 0
    assert skipped <= MAX_SKIPPED, skipped
    assert modes == {"pair", "proband", "ancestor"} and forced >= N_CASES // 3


@pytest.mark.gpu
def test_random_cases_against_the_oracle(gen):
    skipped = 0
    for case in range(N_CASES):
        (args, pro, anc, by), h = plan(gen, case)
        if h is None:
            skipped += 1
            continue
        try:
            h.compute()
            lo, hi, paths, mean = h.result_to_host()
        finally:
            h.close()
        want = DO.depths_exact(*args, pro, anc)
        if by != "pair":
            want = DO.reduce_depths(want, by)
        where = "case %d (%s)" % (case, by)
        assert np.array_equal(paths, want.paths), where
        assert np.array_equal(lo, want.min) and np.array_equal(hi, want.max), where
        assert np.array_equal(mean, want.mean, equal_nan=True), where
    assert skipped <= MAX_SKIPPED, skipped
