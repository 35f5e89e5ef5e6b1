"""The random pedigree generator shared by tests/test_gpu_parity.py, tests/stress_repro.py and tests/stress_sweeps.py."""
import numpy as np


def random_pedigree(rng, n, p_founder, p_one_parent, p_selfing, max_back, max_depth=None):
    """Arbitrary pedigree in id order (parents have smaller ids): overlapping generations,
    one-parent individuals, founders anywhere, occasional selfing, sex not enforced.
    max_depth: an individual whose parents would put it deeper than that many generations is a founder instead
    (drawn the same way: the random stream does not depend on it)."""
    ind = np.arange(1, n + 1, dtype=np.int64)
    fa = np.zeros(n, dtype=np.int64)
    mo = np.zeros(n, dtype=np.int64)
    depth = np.ones(n, dtype=np.int64)
    for i in range(1, n):
        if rng.random() < p_founder:
            continue
        lo = max(0, i - max_back)
        f = int(rng.integers(lo, i)) + 1
        m = int(rng.integers(lo, i)) + 1
        r = rng.random()
        if r < p_one_parent / 2:
            f = 0
        elif r < p_one_parent:
            m = 0
        elif rng.random() < p_selfing:
            m = f
        d = 1 + max(depth[f - 1] if f else 0, depth[m - 1] if m else 0)
        if max_depth is not None and d > max_depth:
            continue
        fa[i], mo[i], depth[i] = f, m, d
    return ind, fa, mo, np.ones(n, dtype=np.int64)
