"""genphi_result_tree over a seeded round of 40 small random pedigrees (tests/random_pedigree.py: overlapping generations, one-parent
individuals, selfing; up to a few hundred probands in any order), with the generators and the knobs of tests/test_clusters_random.py:
for each, three floors drawn from the distinct off-diagonal kinships of its own matrix, 0 and None, the edges against
tests/phi_tree_oracle.py and the rounds against genphi_tree_host on the host copy of the same resident result, and at one threshold
per floor the cut against genphi_result_clusters, ==.  A failing case names its seed."""
import numpy as np
import pytest

import phi_tree_oracle as TO
from random_pedigree import random_pedigree

pytestmark = pytest.mark.gpu

ROUND_CASES, ROUND_SEED, PARTS = 40, 20261021, 4


def _round():
    rng = np.random.default_rng(ROUND_SEED)
    return [int(rng.integers(1 << 30)) for _ in range(ROUND_CASES)]


def _one_case(gen, seed):
    r = np.random.default_rng(seed)
    n = int(r.integers(20, 1200))
    ind, fa, mo, sex = random_pedigree(r, n, p_founder=float(r.choice([0.02, 0.1, 0.3])), p_one_parent=float(r.choice([0.0, 0.1, 0.3])),
                                       p_selfing=float(r.choice([0.0, 0.05])), max_back=int(r.choice([8, 40, 300, n])))
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    kind = int(r.integers(3))
    if kind == 0:
        pro = gen.pro(ped)
    elif kind == 1:
        pro = r.choice(ind, size=int(r.integers(2, min(n, 400) + 1)), replace=False)      # any individuals, in any order
    else:
        pro = r.permutation(ind)[:min(n, 300)]
    what = []
    pl = gen.plan(ped, pro)
    try:
        phi = pl.compute(device=0)
        N = len(phi)
        assert N == pl.n_probands == len(np.unique(pro))
        distinct = np.unique(phi[np.triu_indices(N, 1)]) if N >= 2 else np.zeros(1, dtype=np.float32)
        floors = [float(x) for x in r.choice(distinct, size=3)] + [0.0, None]
        for floor in floors:
            row, col, kin, n_trees, rounds = got = pl.tree(floor)
            want = TO.forest(phi, floor)
            host = gen._capi.tree_host(phi, floor)
            if not TO.same(got, want):
                what.append("floor %r: the edges (%d, oracle %d)" % (floor, len(row), len(want[0])))
            if n_trees != want[3] or n_trees != N - len(row):
                what.append("floor %r: %d trees, oracle %d, %d edges" % (floor, n_trees, want[3], len(row)))
            if not TO.same(host, want):
                what.append("floor %r: the host restatement's edges" % (floor,))
            if rounds != host[4] or rounds > TO.log2_ceil(N) + 1:
                what.append("floor %r: %d rounds, host %d, bound %d" % (floor, rounds, host[4], TO.log2_ceil(N) + 1))
            above = distinct[distinct.astype(np.float64) >= TO.floor_of(floor)]
            if N >= 2 and len(above):
                t = float(r.choice(above))
                k = int(np.count_nonzero(kin.astype(np.float64) >= t))
                label = pl.clusters(t)[0]
                if not np.array_equal(TO.labels_of(N, row[:k], col[:k]), label) or k != N - len(np.unique(label)):
                    what.append("floor %r: the cut at %r against genphi_result_clusters" % (floor, t))
    finally:
        pl.close()
    return ["seed %d (%d individuals, %d probands): %s" % (seed, n, N, w) for w in what]


@pytest.mark.parametrize("part", range(PARTS))
def test_trees_of_random_pedigrees(gen, part):
    """10 of the 40 cases; no case is skipped."""
    seeds = _round()[part::PARTS]
    assert len(seeds) == ROUND_CASES // PARTS
    failures = []
    for seed in seeds:
        print("seed", seed)
        failures += _one_case(gen, seed)
    assert not failures, "\n".join(failures)
