"""genphi_result_clusters / genphi_result_unrelated over a seeded round of 30 small random pedigrees (tests/random_pedigree.py:
overlapping generations, one-parent individuals, selfing; up to a few hundred probands in any order): for each, three thresholds
drawn from the distinct off-diagonal kinships of its own matrix, and 0, both queries and the three priority modes against
tests/phi_clusters_oracle.py on the host copy of the same resident result, ==.  A failing case names its seed."""
import numpy as np
import pytest

import phi_clusters_oracle as CO
from random_pedigree import random_pedigree

pytestmark = pytest.mark.gpu

ROUND_CASES, ROUND_SEED, PARTS = 30, 20261020, 3


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
        thresholds = [float(x) for x in r.choice(distinct, size=3)] + [0.0]
        random_pri = r.integers(-3, 4, N).astype(np.int32)
        for t in thresholds:
            a = CO.adjacency(phi, t)
            label, pairs = pl.clusters(t)
            if not np.array_equal(label, CO.components(a)):
                what.append("threshold %r: labels" % t)
            if pairs != CO.n_pairs(a) or pairs != pl.count_over(t):
                what.append("threshold %r: %d pairs, oracle %d, count_over %d" % (t, pairs, CO.n_pairs(a), pl.count_over(t)))
            for name, pri in (("degree", None), ("position", np.zeros(N, dtype=np.int32)), ("random", random_pri)):
                keep, degree, rounds = pl.unrelated(t, pri)
                jac, ref = CO.jacobi_rounds(a, CO.keys(a, pri))
                if not (np.array_equal(keep, CO.greedy(a, pri)) and np.array_equal(keep, ref)):
                    what.append("threshold %r, by %s: the set" % (t, name))
                if not np.array_equal(degree, CO.degrees(a)):
                    what.append("threshold %r, by %s: degrees" % (t, name))
                if not (N < 2 or 1 <= rounds <= jac):
                    what.append("threshold %r, by %s: %d rounds, synchronous %d" % (t, name, rounds, jac))
    finally:
        pl.close()
    return ["seed %d (%d individuals, %d probands): %s" % (seed, n, N, w) for w in what]


@pytest.mark.parametrize("part", range(PARTS))
def test_clusters_and_unrelated_sets_of_random_pedigrees(gen, part):
    """10 of the 30 cases; no case is skipped."""
    seeds = _round()[part::PARTS]
    assert len(seeds) == ROUND_CASES // PARTS
    failures = []
    for seed in seeds:
        print("seed", seed)
        failures += _one_case(gen, seed)
    assert not failures, "\n".join(failures)
