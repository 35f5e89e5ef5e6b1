"""genphi_result_matmul over every path that delivers the resident result: 20 cases drawn with tests/stress_queries.make_case (imported,
not edited) and walked through their resident states as stress_queries.run_case walks them -- a soiled device cache, FULL / SPLIT / WIDE
last steps, in-place delivery, unaligned / one-row / last-row / empty shards, kernel = 1, no_sparse, a Float64 state in between,
release_device.  After every Float32 state an exact-integer product is compared with the host copy of the same state, bit for bit, after
the exactness condition of tests/test_phi_matmul_gpu.py has been asserted on that copy; after a Float64 state the product is refused.
What the product relies on and no interface states is what the other queries rely on: padding columns [N, ld) of +0 after
every delivery path, ld % 64 == 0, and the resident row range following every compute."""
import numpy as np
import pytest

import stress_queries as S
from test_phi_matmul_gpu import exact_condition, same

N_CASES, SEED = 20, 20261118
WIDTHS = [1, 2, 3, 5, 8, 9, 17, 64]


def _cases():
    rng = np.random.default_rng(SEED)
    return [int(rng.integers(1 << 30)) for _ in range(N_CASES)]


def test_the_cases_are_a_pure_function_of_their_numbers_and_cover_the_states():
    """No GPU: the 20 cases hold every kind of state the walk is about, at least once."""
    kinds, soiled, n_f32 = set(), 0, 0
    for case in _cases():
        c = S.make_case(case)
        assert S.describe(c) == S.describe(S.make_case(case))
        soiled += c["soil"]
        for s in c["states"]:
            kinds.add(s["kind"])
            n_f32 += not s["f64"]
            a, b = S.rows_of(s, c["n"])
            if a == b:
                kinds.add("an empty shard")
    assert {"full", "shard", "one_row", "last_row", "an empty shard", "kernel1", "no_sparse", "f64", "f32_after_f64", "release_then_compute"} <= kinds, kinds
    assert soiled >= 3 and n_f32 >= 50


@pytest.mark.gpu
@pytest.mark.parametrize("case", _cases())
def test_product_after_every_delivery(gen, case):
    c = S.make_case(case)
    n = c["n"]
    ind, fa, mo, sex = c["ind"], c["father"], c["mother"], c["sex"]
    if not c["sort"]:
        from genlib_jl_amd import synth
        ind, fa, mo, sex = synth.parents_first_shuffle(ind, fa, mo, sex, seed=c["base"] & 0xffff)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}, sort=c["sort"])
    if c["soil"]:
        assert S.soil(gen, n)
    rng = np.random.default_rng([case, 19])
    pl = gen.plan(ped, c["pro"], tuning=c["tuning"])
    try:
        for i, s in enumerate(c["states"]):
            r0, r1 = S.rows_of(s, n)
            if s["release"]:
                pl.release_device()
            pl.compute_device(kernel=s["kernel"], rows=s["rows"], storage64=s["f64"], no_sparse=s["no_sparse"])
            k = int(rng.choice(WIDTHS))
            X = rng.integers(-1000, 1001, size=(n, k)).astype(np.float64)
            if s["f64"]:
                with pytest.raises(ValueError, match="Float32"):
                    pl.matmul(X)
                continue
            host = pl.result_to_host()
            assert host.shape == (r1 - r0, n), (i, S.show_state(s))
            exact_condition(host, X)
            got = pl.matmul(X)
            assert same(got, host.astype(np.float64) @ X), (i, S.show_state(s), k)
            assert same(pl.matmul(X[:, k - 1]), np.ascontiguousarray(got[:, k - 1])), (i, S.show_state(s), k)
    finally:
        pl.close()
