"""A random differential round for gen.simuSegments on the MI355X: 30 cases, each a pedigree and an ID map of tests/stress_drops.py
(cut to its first individuals, parents come before children), random probands with repeats, L at the word edges, q from the kinds
of the definition, S, a forced panel width, random edges, min_loci and labels; the table and the pair sums of
gen.SharingPlan.request_segments against tests/segments_oracle.py by np.array_equal, computed twice.  The cases are drawn on the
host from the case number alone, and a test without a GPU asserts what they reach."""
import numpy as np
import pytest

from link_oracle import LinkVector, sums_of
from segments_oracle import segments_of
from stress_drops import _id_map, _pedigree
from test_segments_host import check_oracle_invariants

N_CASES = 30
MAX_IND = 260                 # the reference holds Int32 labels of everyone: individuals x 2 x S x L
LOCI = [1, 63, 64, 65, 128, 129, 191]
QS = [0, 1, 64, 700, 0x5555, 32768]
SIMS = [1, 2, 3, 65]


def make_case(case):
    r = np.random.default_rng([2027, case])
    kind, fa, mo, _ = _pedigree(r, case)
    n = min(len(fa), int(r.integers(8, MAX_IND + 1)))
    fa, mo = fa[:n], mo[:n]
    new = _id_map(r, str(r.choice(["small", "high", "low_shared", "high_shared"])), fa, mo)
    ind, fa, mo = new[1:], new[fa], new[mo]
    n_pro = int(r.choice([1, 2, 5, 17, 33, 40]))
    pro = r.choice(ind[n // 2:], size=n_pro, replace=True).astype(np.int64)     # the later generations, with repeats
    S = int(r.choice(SIMS))
    L = int(r.choice(LOCI if S < 65 else LOCI[:6]))
    q = int(r.choice(QS))
    panel = int(r.choice([0, 1, 2, S + 3])) if S > 1 else int(r.choice([0, 1]))
    n_edges = int(r.integers(2, 12))
    edges = np.sort(r.choice(np.arange(1, L + 3), size=min(n_edges, L + 2), replace=False))
    if len(edges) < 2:
        edges = np.array([1, 2])
    if case % 3 == 0:
        edges = edges[edges <= max(L // 2, 2)] if (edges <= max(L // 2, 2)).sum() >= 2 else np.array([1, 2])      # lengths at and above the last edge
    groups = None
    if r.random() < 0.5:
        G = int(r.integers(1, 6))
        groups = r.integers(-1, G, size=n_pro)
        groups[int(r.integers(0, n_pro))] = G - 1                               # the table has G groups
    return dict(kind=kind, ind=ind, fa=fa, mo=mo, pro=pro, S=S, L=L, q=q, panel=panel, edges=edges.astype(np.int32),
                min_loci=int(r.choice([1, 2, 64, 65, L, L + 1])), groups=groups, seed=int(r.integers(0, 1 << 63)) * 2 + int(r.integers(0, 2)),
                all_pairs=bool(r.integers(0, 2)))


def panels_of(c):
    sims = c["S"] if c["panel"] == 0 else min(c["panel"], c["S"])
    return (c["S"] + sims - 1) // sims


@pytest.fixture(scope="module")
def cases():
    return [make_case(k) for k in range(N_CASES)]


@pytest.fixture(scope="module")
def references(cases):
    """Per case (labels, hist, pairs) of the reference, held against link_oracle.sums_of first; computed once for both tests."""
    out = []
    for c in cases:
        want = LinkVector(c["ind"], c["fa"], c["mo"], c["pro"]).labels(c["S"], c["L"], c["q"], c["seed"])
        check_oracle_invariants(want, c["edges"], c["groups"])
        out.append((want,) + segments_of(want, c["edges"], c["min_loci"], c["groups"]))
    return out


def test_what_the_cases_reach(cases, references):
    """On the host, from the draws and the reference: grouped and ungrouped tables that are not empty, more than one panel, a
    non-empty `above`, `below` and bins, every S, q and word count."""
    hists = [hist for _, hist, _ in references]
    upper = [hist[np.triu(np.ones(hist.shape[:2], dtype=bool))] for hist in hists]
    assert sum(int(u[:, -1, 0].sum() > 0) for u in upper) >= 3                            # `above`
    assert sum(int(u[:, 0, 0].sum() > 0) for u in upper) >= 3 and sum(int(u[:, 1:-1, 0].sum() > 0) for u in upper) >= 5
    assert sum(int(c["groups"] is not None and u[..., 0].sum() > 0) for c, u in zip(cases, upper)) >= 3
    assert sum(int(c["groups"] is None and u[..., 0].sum() > 0) for c, u in zip(cases, upper)) >= 3
    assert any(c["groups"] is not None and c["groups"].max() >= 1 and u[1:, :, 0].sum() > 0 for c, u in zip(cases, upper))      # a second pair of groups counts
    assert sum(int(u[..., 0].sum()) for u in upper) > 1000 and any(u[..., 2].sum() < u[..., 0].sum() for u in upper)              # uncensored segments
    assert sum(int(panels_of(c) > 1 and u[..., 0].sum() > 0) for c, u in zip(cases, upper)) >= 3                                  # panels that add up
    assert any(c["groups"] is not None for c in cases) and any(c["groups"] is None for c in cases)
    assert any(c["groups"] is not None and (c["groups"] < 0).any() for c in cases)
    assert sum(panels_of(c) > 1 for c in cases) >= 5 and any(panels_of(c) == 1 for c in cases)
    assert {c["S"] for c in cases} == set(SIMS) and {c["q"] for c in cases} == set(QS)
    assert {(c["L"] + 63) // 64 for c in cases} == {1, 2, 3} and any(c["L"] % 64 not in (0, 1, 63) or c["L"] in (1, 63) for c in cases)
    assert any(c["all_pairs"] for c in cases) and not all(c["all_pairs"] for c in cases)
    assert any(len(c["pro"]) > 32 for c in cases) and any(len(np.unique(c["pro"])) < len(c["pro"]) for c in cases)
    assert any(c["edges"][-1] <= c["L"] for c in cases) and any(c["min_loci"] > 1 for c in cases)


@pytest.mark.gpu
def test_random_round(gen, cases, references):
    above = grouped = several = segments = 0
    for k, (c, (want, hist, pairs)) in enumerate(zip(cases, references)):
        args = (c["ind"], c["fa"], c["mo"])
        h = gen.SharingPlan(*args, c["pro"], loci=c["L"], q=c["q"], simul_no=c["S"], seed=c["seed"], panel_sims=c["panel"], all_pairs=c["all_pairs"])
        try:
            h.request_segments(c["edges"], c["min_loci"], c["groups"])
            for _ in range(2):
                h.compute()
                got_hist, got_pairs = h.segments_to_host()
                note = (k, c["kind"], len(c["pro"]), c["S"], c["L"], c["q"], c["panel"], c["edges"].tolist(), c["min_loci"])
                assert got_hist.shape == hist.shape and np.array_equal(got_hist, hist), note
                assert np.array_equal(got_pairs, pairs), note
                assert np.array_equal(h.sums_to_host(), sums_of(want)), note
            assert h.stats()["panels"] == panels_of(c)
            several += panels_of(c) > 1
        finally:
            h.close()
        above += int(hist[..., -1, 0].sum() > 0)
        grouped += int(c["groups"] is not None and hist[..., 0].sum() > 0)
        segments += int(hist[np.triu(np.ones(hist.shape[:2], dtype=bool))][..., 0].sum())
    print("random round: %d cases, %d segments, %d with a non-empty above, %d grouped and non-empty, %d with several panels" % (
        len(cases), segments, above, grouped, several))
    assert above >= 3 and grouped >= 3 and several >= 5 and segments > 1000
