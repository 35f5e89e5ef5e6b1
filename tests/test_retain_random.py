"""A random differential round for gen.simuRetention on the MI355X: 40 cases, each a pure function of its number, against the
reference of tests/retain_oracle.py with np.array_equal.  Pedigrees of tests/random_pedigree.py of at most 1,500 individuals, IDs
mapped into [2^40, 2^62) in some cases, seeds with high bits set, proband lists that mix leaves, inner individuals, founders and
repeats, S at word edges, forced and ragged panels and label chunks, both forms of the mark phase.  n_ind x S <= 3 x 10^6, the cost
of the reference (as in tests/stress_drops.py).  A host-side test asserts that the cases reach more than one chunk, more than one
panel and a founder split by a chunk border."""
import numpy as np
import pytest

from ident_oracle import IdentVector
from random_pedigree import random_pedigree
from retain_oracle import check_invariants, reductions

CASES = list(range(40))
ROWS_CAP = 3_000_000
S_EDGES = [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 640, 1000, 2000, 5000]


def make_case(case):
    r = np.random.default_rng([20261020, case])
    n = int(r.choice([5, 40, 150, 400, 900, 1500]))
    n = max(2, n - int(r.integers(0, 4)))
    ind, fa, mo, _ = random_pedigree(r, n, p_founder=float(r.choice([0.05, 0.15, 0.4])), p_one_parent=float(r.choice([0.0, 0.1, 0.3])),
                                     p_selfing=float(r.choice([0.0, 0.05])), max_back=int(r.choice([5, 40, 400])))
    big_ids = case % 3 == 0
    if big_ids:                                                                 # an increasing map: the order of the table stays
        new = np.sort(r.integers(2**40, 2**62, size=n, dtype=np.int64))
        assert len(np.unique(new)) == n
        lookup = np.concatenate([[0], new])                                     # (ind is 1 .. n: an ID is its own position + 1)
        fa, mo, ind = lookup[fa], lookup[mo], new
    S = int(r.choice([s for s in S_EDGES if n * s <= ROWS_CAP]))
    n_pro = int(r.choice([1, 2, 7, 15, 16, 17, 33, 100, 300, 300]))
    kind = int(r.integers(0, 3))
    pool = ind if kind == 0 else (ind[len(ind) // 2:] if kind == 1 else ind[~np.isin(ind, np.union1d(fa, mo))])
    if len(pool) == 0:
        pool = ind
    pro = r.choice(pool, size=n_pro, replace=True).astype(np.int64)
    seed = int(r.integers(0, 2**63)) | (1 << 63 if case % 2 else 1 << 31)
    panel = int(r.choice([0, 0, 128, 129, 384, 1000, 100000]))
    chunk = int(r.choice([0, 1, 32, 32, 33, 64, 64, 96, 4096]))
    mark = [None, "or", "test"][case % 3 if case % 2 else 0]
    return dict(ind=ind, fa=fa, mo=mo, pro=pro, S=S, seed=seed, panel=panel, chunk=chunk, mark=mark, big_ids=big_ids)


def shape(c, alleles):
    """(chunks, panels, a founder split by a chunk border, a ragged last chunk) as the rules of csrc/retain.h and csrc/drop_plan.h give them."""
    n = len(alleles)
    lc = min(n, 16384, (c["chunk"] + 31) // 32 * 32 if c["chunk"] else 8192)
    total = -(-c["S"] // 128)
    pn = min(total, -(-c["panel"] // 128)) if c["panel"] else total
    borders = np.arange(lc, n, lc)
    split = bool(len(borders)) and bool(np.any(alleles[borders - 1, 0] == alleles[borders, 0]))
    return -(-n // lc), -(-total // pn), split, n % lc != 0


def test_the_cases_reach_what_they_claim():
    chunks = panels = splits = ragged = big = high = 0
    marks, sizes = set(), set()
    for case in CASES:
        c = make_case(case)
        again = make_case(case)
        assert all(np.array_equal(c[k], again[k]) for k in c), case                       # a pure function of its number
        assert len(c["ind"]) <= 1500 and len(c["ind"]) * c["S"] <= ROWS_CAP
        o = IdentVector(c["ind"], c["fa"], c["mo"], c["pro"])
        k, p, split, rag = shape(c, o.alleles)
        chunks += k > 1
        panels += p > 1
        splits += split
        ragged += rag and k > 1
        big += c["big_ids"] and int(c["ind"].min()) >= 2**40
        high += c["seed"] >= 2**63
        marks.add(c["mark"])
        sizes.add(c["S"] % 64)
    assert chunks >= 5 and panels >= 5 and splits >= 2 and ragged >= 3 and big >= 10 and high >= 15 and marks == {None, "or", "test"}
    assert len(sizes) >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_random_case(gen, case):
    c = make_case(case)
    args = (c["ind"], c["fa"], c["mo"])
    o = IdentVector(*args, c["pro"])
    want = reductions(o.labels(c["S"], c["seed"]), o.alleles)
    h = gen.RetentionPlan(*args, c["pro"], simul_no=c["S"], seed=c["seed"], panel_cols=c["panel"], chunk_labels=c["chunk"], mark=c["mark"])
    try:
        assert np.array_equal(h.alleles(), o.alleles) and h.seed == c["seed"]
        for _ in range(2):
            h.compute()
            got = h.survived_to_host(), h.both_to_host(), h.distinct_to_host()
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (case, np.argwhere(g != w)[:5])
        check_invariants(*got, o.alleles, c["S"], c["pro"])
        st = h.stats()
        k, p, _, _ = shape(c, o.alleles)
        assert (st["chunks"], st["panels"]) == (k, p)
    finally:
        h.close()
