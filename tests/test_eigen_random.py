"""genphi_result_eigen over every path that delivers the resident result: 20 cases drawn with tests/stress_queries.make_case (imported,
not edited) and walked through their resident states as tests/test_matmul_random.py walks them.  After every FULL Float32 state the
k = min(3, N) largest pairs are compared with numpy.linalg.eigh of the host copy of the same state; after a shard and after a Float64
state the call is refused.  The cases hold unrelated founders and duplicated probands, so eigenvalues repeat: the checks are those of
tests/test_phi_eigen_gpu.py that need no simple spectrum -- every pair lies within its true residual (plus rounding) of SOME eigenvalue,
no Ritz value exceeds the eigenvalue of its rank, the first one is the largest eigenvalue, flagged pairs meet the tolerance, and the
vectors are orthonormal -- and the per-rank comparison where the top k + 1 eigenvalues are simple."""
import numpy as np
import pytest

import stress_queries as S
from test_phi_eigen_gpu import TOL, U, rounding

N_CASES, SEED = 20, 20261019


def _cases():
    rng = np.random.default_rng(SEED)
    return [int(rng.integers(1 << 30)) for _ in range(N_CASES)]


def test_the_cases_cover_full_states_shards_and_float64():
    """No GPU: the 20 cases hold full Float32 states, shards and Float64 states."""
    full = shard = f64 = 0
    for case in _cases():
        c = S.make_case(case)
        assert S.describe(c) == S.describe(S.make_case(case))
        for s in c["states"]:
            f64 += s["f64"]
            full += not s["f64"] and S.rows_of(s, c["n"]) == (0, c["n"])
            shard += not s["f64"] and S.rows_of(s, c["n"]) != (0, c["n"])
    assert full >= 20 and shard >= 10 and f64 >= 5, (full, shard, f64)


@pytest.mark.gpu
@pytest.mark.parametrize("case", _cases())
def test_eigenpairs_after_every_delivery(gen, case):
    c = S.make_case(case)
    n = c["n"]
    ind, fa, mo, sex = c["ind"], c["father"], c["mother"], c["sex"]
    if not c["sort"]:
        from genlib_jl_amd import synth
        ind, fa, mo, sex = synth.parents_first_shuffle(ind, fa, mo, sex, seed=c["base"] & 0xffff)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}, sort=c["sort"])
    if c["soil"]:
        assert S.soil(gen, n)
    pl = gen.plan(ped, c["pro"], tuning=c["tuning"])
    k = min(3, n)
    try:
        for i, s in enumerate(c["states"]):
            r0, r1 = S.rows_of(s, n)
            if s["release"]:
                pl.release_device()
            pl.compute_device(kernel=s["kernel"], rows=s["rows"], storage64=s["f64"], no_sparse=s["no_sparse"])
            where = (i, S.show_state(s))
            if s["f64"]:
                with pytest.raises(ValueError, match="Float32"):
                    pl.eigen(k)
                continue
            if (r0, r1) != (0, n):
                with pytest.raises(ValueError, match="shard"):
                    pl.eigen(k)
                continue
            host = pl.result_to_host().astype(np.float64)
            assert host.shape == (n, n), where
            lam = np.linalg.eigvalsh(host)[::-1]
            val, vec, res, conv, m = pl.eigen(k, False, TOL, seed=case)
            r = rounding(n, m, val[0])
            assert np.all(conv) and 1 <= m <= n, where
            assert np.all(res <= TOL * val[0] + r), (where, res)
            assert np.all(np.abs(lam[None, :] - val[:, None]).min(axis=1) <= res + r), (where, val)
            assert np.all(val <= lam[:k] + r) and np.all(np.diff(val) <= r) and abs(val[0] - lam[0]) <= res[0] + r, (where, val, lam[:k])
            assert np.abs(vec.T @ vec - np.eye(k)).max() <= (m + 2) * (n + 2) * U, where
            if np.all(-np.diff(lam[:min(k + 1, n)]) > 2 * TOL * lam[0]):
                assert np.all(np.abs(val - lam[:k]) <= res + r), (where, val, lam[:k])
    finally:
        pl.close()
