"""The queries on the resident result (genphi_result_sums, _group_sums, _over, _nearest, _bootstrap) over every path that delivers that
result: a short fixed-seed round of tests/stress_queries.py, what that round is guaranteed to contain (checked on the host alone), and
three pinned deliveries on their smallest shapes.  Every comparison is with the Python oracles of tests/*_oracle.py on the host copy of
the same result; the only tolerances are the two derived ones named in tests/stress_queries.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import phi_ci_oracle as CO
import stress_queries as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROUND_CASES, ROUND_SEED = 60, 20261021


def _round():
    rng = np.random.default_rng(ROUND_SEED)
    return [int(rng.integers(1 << 30)) for _ in range(ROUND_CASES)]


@pytest.mark.gpu
def test_query_stress_short():
    """60 fixed-seed cases of tests/stress_queries.py: the pedigrees, proband lists and sweep knobs of tests/stress_random.py (at most 400
    probands, 7,000 individuals) x a soiled device cache x 3 - 6 resident states on one plan x all five queries against their oracles.
    No case is skipped.  Measured on an MI355X machine the whole round takes 5.2 - 5.8 s of wall time (three runs), with 14 s of CPU in the
    oracles (summed over the threads of the compiled one)."""
    out = subprocess.run([sys.executable, os.path.join(HERE, "stress_queries.py"), str(ROUND_CASES), str(ROUND_SEED)], cwd=HERE, capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    last = out.stdout.splitlines()[-1]
    assert last.startswith("query stress: %d cases, 0 failures" % ROUND_CASES), out.stdout[-3000:]
    assert ", 0 failures" in last


@pytest.mark.gpu
@pytest.mark.parametrize("case", [822667127, 412805880, 705161730])
def test_query_cases_that_failed_once(gen, oracle, case):
    """Cases of the first round: an empty shard between two results (its row pitch was reported as 0, and genphi_result_group_sums
    called it "no resident result"), an empty shard as the first state, and an empty Float32 shard right after a Float64 result
    (the plan went on calling the result Float64, so every query and the host copy refused it)."""
    what, c = S.run_case(case, gen, oracle)
    assert any(a == b for a, b in (S.rows_of(s, c["n"]) for s in c["states"]))
    assert not what, what


def classes_of(gen, c):
    """The classes of the coverage test that one case belongs to, from the plan's accessors on the host and the state list."""
    ind, fa, mo, sex = c["ind"], c["father"], c["mother"], c["sex"]
    if not c["sort"]:
        from genlib_jl_amd import synth
        ind, fa, mo, sex = synth.parents_first_shuffle(ind, fa, mo, sex, seed=c["base"] & 0xffff)
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}, sort=c["sort"])
    pl = gen.plan(ped, c["pro"], tuning=c["tuning"])
    try:
        n, modes, sizes = pl.n_probands, pl.step_modes(), pl.levels()[0]
        in_place = bool(modes) and bool(pl.step_slots(len(modes) - 1)[0] & 1)
    finally:
        pl.close()
    assert n == c["n"] and sizes[-1] == n and len(modes) == len(sizes) - 1
    assert 3 <= len(c["states"]) <= 6 and not c["states"][-1]["f64"]
    rows = [S.rows_of(s, n) for s in c["states"]]
    assert all(0 <= a <= b <= n for a, b in rows)
    out = set()
    if not modes:
        out.add("no level step")
    elif in_place:
        out.add("last step in place")
    else:
        out.add(["last step FULL", "last step SPLIT", "last step WIDE, proband-order pass"][modes[-1]])
    if n % 4:
        out.add("N % 4 != 0")
    if n % 64 == 0:
        out.add("N % 64 == 0")
    if n == 2:
        out.add("N == 2")
    if any(a % 4 and b > a and not s["f64"] for s, (a, b) in zip(c["states"], rows)):
        out.add("shard off a multiple of 4")
    if any(a == b for a, b in rows):
        out.add("empty shard")
    if any(s["kernel"] == 1 for s in c["states"]):
        out.add("kernel=1")
    if any(s["f64"] for s in c["states"][:-1]):
        out.add("Float64 state in the middle")
    if c["soil"]:
        out.add("soiled cache")
    return out


CLASSES = ["last step FULL", "last step SPLIT", "last step WIDE, proband-order pass", "last step in place", "no level step", "N % 4 != 0",
           "N % 64 == 0", "N == 2", "shard off a multiple of 4", "empty shard", "kernel=1", "Float64 state in the middle", "soiled cache"]


def test_the_short_round_reaches_every_delivery_path(gen):
    """No GPU: the plan of every case of the fixed-seed round, built on the host, and its state list.  At least 3 cases of every class."""
    seen = {k: 0 for k in CLASSES}
    for case in _round():
        c = S.make_case(case)
        again = S.make_case(case)                                          # a pure function of the case number
        assert S.describe(c) == S.describe(again) and np.array_equal(c["pro"], again["pro"]) and c["seed"] == again["seed"]
        assert c["n"] <= S.MAX_PRO and len(c["ind"]) <= S.MAX_IND
        for k in classes_of(gen, c):
            seen[k] += 1
    print(seen)
    assert all(v >= 3 for v in seen.values()), seen


def test_the_soiling_pedigree_has_no_zero_kinship(oracle):
    ind, fa, mo, pro = S.soiling_pedigree(37)
    phi = oracle.Pedigree(ind, fa, mo, sort=False).phi(pro)
    assert phi.shape == (37, 37) and np.all(phi > 0)


# ---- pinned deliveries ------------------------------------------------------------------------------------------------------------

def _all_queries(gen, oracle, ind, fa, mo, sex, pro, tuning, shard, expect):
    """Soil the cache, then the full result and one unaligned shard of (pedigree, pro) under `tuning`: host copy and all five queries.
    expect(plan) asserts that the plan takes the delivery path the test is about."""
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex})
    want = oracle.Pedigree(ind, fa, mo).phi(pro)
    n = len(want)
    assert S.soil(gen, n)
    c = dict(n=n, seed=0x9E3779B97F4A7C15)
    counts = {}
    pl = gen.plan(ped, pro, tuning=tuning)
    try:
        expect(pl)
        for rows in (None, shard, None):
            assert rows is None or (0 < rows[0] < rows[1] <= n and rows[0] % 4 and rows[1] % 4)
            s = dict(kind="pinned", rows=rows, kernel=0, no_sparse=False, f64=False, release=False, k=min(n - 1, 64), G=7, label_seed=n, b=65,
                     entry=(0.37, 0.61))
            r0, r1 = S.rows_of(s, n)
            pl.compute_device(device=0, rows=rows)
            host = pl.result_to_host()
            assert np.array_equal(host.view(np.int32), want[r0:r1].view(np.int32))
            _, ld, rb, nr = pl.result_device()
            assert (rb, nr) == (r0, r1 - r0) and ld % 64 == 0 and ld >= n
            what, lines = [], []
            S.check_queries(gen, pl, c, s, host, what, lines.append, lambda b: counts.setdefault(b, CO.counts(n, c["seed"], 0, b)))
            assert not what, "\n".join(lines)
    finally:
        pl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("plain", [False, True])
def test_queries_after_a_wide_last_step(gen, oracle, plain):
    """A WIDE last step (an LDS budget of 256 floats on 300 probands) delivered by the proband-order pass: the persistent form, and the
    one-workgroup-per-row form (GENPHI_COLPERM_PLAIN)."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, pro = synth.random_mating(3000, 300, 12, skip_permille=100, seed=11)
    tuning = {"LDS_CAP_FLOATS": 256, "STAY_LAST": 0}
    if plain:
        tuning["COLPERM_PLAIN"] = 1

    def expect(pl):
        last = len(pl.step_modes()) - 1
        assert pl.step_modes()[last] == 2 and not pl.step_slots(last)[0] & 1

    _all_queries(gen, oracle, ind, fa, mo, sex, pro, tuning, (101, 203), expect)


@pytest.mark.gpu
def test_queries_after_a_delivery_from_the_slot_matrix(gen, oracle):
    """Every individual of a small pedigree with overlapping generations is a proband: the proband cut stays in place and the result is
    delivered from the slot matrix (Plan::final_slots)."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, _ = synth.random_mating(500, 30, 5, skip_permille=400, seed=1)
    tuning = {"LDS_CAP_FLOATS": 256, "STAY_MEM_PCT": 100000, "STAY_NARROW_MIN": 0, "STAY_OVERHEAD_K": 0}

    def expect(pl):
        last = len(pl.step_modes()) - 1
        assert pl.step_modes()[last] == 2 and pl.step_slots(last)[0] & 1

    _all_queries(gen, oracle, ind, fa, mo, sex, ind.copy(), tuning, (101, 331), expect)


@pytest.mark.gpu
def test_queries_on_founders_only(gen, oracle):
    """37 founders and a repeat: no level step, the result is 1/2 I written by the identity kernel."""
    from genlib_jl_amd import synth
    ind, fa, mo, sex, _ = synth.random_mating(600, 50, 5, seed=2)
    founders = ind[(fa == 0) & (mo == 0)][:37]
    assert len(founders) == 37

    def expect(pl):
        assert pl.step_modes() == [] and pl.n_probands == 37

    _all_queries(gen, oracle, ind, fa, mo, sex, np.concatenate([founders, founders[3:4]]), {}, (5, 30), expect)
