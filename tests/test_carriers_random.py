"""A random differential round for gen.simuCarriers on the MI355X: 40 cases, each a pure function of its number, against the
reference of tests/carriers_oracle.py with np.array_equal.  Pedigrees, ID maps (small IDs, IDs in [2^40, 2^62), groups that share a
low or a high half), seeds with high halves, and the simulations at the word and pair edges with forced and ragged panels are drawn
with the generators of tests/stress_drops.py; on top of them mixed lists of cases and controls (leaves, inner individuals,
founders, repeats), forced and ragged label chunks and max_count.  n_ind x S <= 3 x 10^6, the cost of the reference.  A host-side test
asserts that the drawn cases reach every class: with and without controls, lumped and full width, more than one chunk, more than one
panel."""
import numpy as np
import pytest

from carriers_oracle import CarryVector, check_invariants
from stress_drops import ID_MAPS, SEED_KINDS, _id_map, _pedigree, _sims_and_panel, panel_pairs

CASES = list(range(40))
ROWS_CAP = 3_000_000
DEFAULT_CHUNK = 608                          # csrc/carry.h: CARRY_DEFAULT_CHUNK
MAX_CHUNK = 608                              # csrc/carry.h: CARRY_MAX_CHUNK


def make_case(case):
    r = np.random.default_rng([20261021, case])
    _, fa, mo, _ = _pedigree(r, case)
    n = len(fa)
    ind = np.arange(1, n + 1, dtype=np.int64)
    parents = np.union1d(fa, mo)
    leaves = np.setdiff1d(ind, parents)
    founders = ind[(fa == 0) & (mo == 0)]
    inner = np.setdiff1d(np.setdiff1d(ind, leaves), founders)

    def some(pool, k):
        return r.choice(pool, size=min(int(k), len(pool)), replace=False) if len(pool) and k > 0 else np.zeros(0, dtype=np.int64)

    n_cases = int(r.choice([1, 2, 7, 15, 16, 17, 33, 63, 64, 65, 100, 200]))
    cases = np.concatenate([some(leaves, n_cases), some(inner, r.integers(0, 6)), some(founders, r.integers(0, 3))]).astype(np.int64)
    if len(cases) == 0:
        cases = ind[-1:].copy()
    with_controls = case % 3 != 0
    controls = np.zeros(0, dtype=np.int64)
    if with_controls:
        rest = np.setdiff1d(ind, cases)
        controls = np.concatenate([some(np.intersect1d(rest, leaves), r.integers(1, 20)), some(np.intersect1d(rest, inner), r.integers(0, 4)),
                                   some(np.intersect1d(rest, founders), r.integers(0, 3))]).astype(np.int64)
    if case % 2:                                                                # repeats and another order
        cases = r.permutation(np.concatenate([cases, r.choice(cases, size=int(r.integers(1, 5)))]))
        if len(controls):
            controls = r.permutation(np.concatenate([controls, controls[:2]]))
    S, panel, _ = _sims_and_panel(r, max(1, min(65, ROWS_CAP // n // 128)))
    n_distinct = len(np.unique(cases))
    max_count = int(r.choice([0, 0, 1, 2, 3, max(1, n_distinct - 1), n_distinct, n_distinct + 5]))
    chunk = int(r.choice([0, 0, 1, 32, 32, 33, 64, 64, 96, 128, 256, 4096]))
    id_map = str(r.choice(ID_MAPS))
    new = _id_map(r, id_map, fa, mo)
    ind, fa, mo, cases, controls = new[ind], new[fa], new[mo], new[cases], new[controls]
    seed_kind = str(r.choice(SEED_KINDS[1:]))                                   # every seed has a high half
    seed = {"high_half": int(r.integers(1, 1 << 32)) << 32, "top_bit": int(r.integers(1 << 63, 1 << 64, dtype=np.uint64)),
            "all_ones": (1 << 64) - 1}[seed_kind]
    return dict(ind=ind, fa=fa, mo=mo, cases=cases, controls=controls, S=S, seed=seed, panel=panel, chunk=chunk, max_count=max_count, id_map=id_map)


def shape(c, n_labels):
    """(chunks, a ragged last chunk, panels, a ragged last panel, lumped) as the rules of csrc/carry.h and csrc/drop_plan.h give them."""
    lc = min(n_labels, MAX_CHUNK, (c["chunk"] + 31) // 32 * 32 if c["chunk"] else DEFAULT_CHUNK)
    pn, panels = panel_pairs(c["S"], c["panel"])
    n = len(np.unique(c["cases"]))
    return -(-n_labels // lc), n_labels % lc != 0, panels, -(-c["S"] // 128) % pn != 0, 0 < c["max_count"] < n


def test_the_cases_reach_what_they_claim():
    from ident_oracle import IdentVector
    chunks = ragged = panels = ragged_panels = lumped = full = controls = plain = high = repeats = 0
    maps, sizes = set(), set()
    for case in CASES:
        c = make_case(case)
        again = make_case(case)
        assert all(np.array_equal(c[k], again[k]) for k in c), case                       # a pure function of its number
        assert len(c["ind"]) * c["S"] <= ROWS_CAP and len(np.unique(c["cases"])) <= 32767
        assert not np.any(np.isin(c["controls"], c["cases"])) and c["seed"] >= 2**32
        o = IdentVector(c["ind"], c["fa"], c["mo"], np.concatenate([c["cases"], c["controls"]]))
        k, rag, p, rag_p, lump = shape(c, o.n_labels)
        chunks += k > 1
        ragged += rag and k > 1
        panels += p > 1
        ragged_panels += rag_p
        lumped += lump
        full += not lump
        controls += len(c["controls"]) > 0
        plain += len(c["controls"]) == 0
        high += c["seed"] >= 2**63
        repeats += len(np.unique(c["cases"])) < len(c["cases"])
        maps.add(c["id_map"])
        sizes.add(c["S"] % 64)
    assert chunks >= 5 and ragged >= 3 and panels >= 5 and ragged_panels >= 3 and lumped >= 8 and full >= 8 and controls >= 20 and plain >= 10
    assert high >= 10 and repeats >= 15 and maps == set(ID_MAPS) and len(sizes) >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_random_case(gen, case):
    c = make_case(case)
    args = (c["ind"], c["fa"], c["mo"])
    ref = CarryVector(*args, c["cases"], c["controls"], c["S"], c["seed"])
    want = ref.at(c["S"], c["max_count"])
    h = gen.CarriersPlan(*args, c["cases"], c["controls"], simul_no=c["S"], seed=c["seed"], panel_cols=c["panel"], chunk_labels=c["chunk"],
                         max_count=c["max_count"])
    try:
        assert np.array_equal(h.alleles(), ref.alleles) and h.seed == c["seed"]
        assert (h.n_cases, h.n_controls, h.columns) == (ref.n, len(ref.control_labels), want[0].shape[1])
        for _ in range(2):
            h.compute()
            got = h.carriers_to_host(), h.homozygotes_to_host(), h.excluded_to_host()
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (case, np.argwhere(g != w)[:5])
        check_invariants(*got, ref.alleles, c["S"], c["cases"], c["controls"])
        st = h.stats()
        k, _, p, _, _ = shape(c, ref.n_labels)
        assert (st["chunks"], st["panels"]) == (k, p)
    finally:
        h.close()
