"""A random differential round for gen.simuOrigins on the MI355X: 40 cases, each a pure function of its number, against the reference
of tests/origins_oracle.py with np.array_equal.  Pedigrees, ID maps (small IDs, IDs in [2^40, 2^62), groups that share a low or a high
half), seeds with high halves, and the simulations at the word and pair edges with forced and ragged panels are drawn with the
generators of tests/stress_drops.py; on top of them mixed lists of probands (leaves, inner individuals, founders, repeats), random
groups with -1 and empty groups, forced and ragged label chunks, and the table by proband on and off.  n_ind x S <= 3 x 10^6, the cost
of the reference.  A host-side test asserts that the drawn cases reach every class: one group and more than eight, more than one
chunk, more than one panel, by proband on and off."""
import numpy as np
import pytest

from origins_oracle import OriginVector, check_invariants
from stress_drops import ID_MAPS, SEED_KINDS, _id_map, _pedigree, _sims_and_panel, panel_pairs

CASES = list(range(40))
ROWS_CAP = 3_000_000


def make_case(case):
    r = np.random.default_rng([20261022, case])
    _, fa, mo, _ = _pedigree(r, case)
    n = len(fa)
    ind = np.arange(1, n + 1, dtype=np.int64)
    parents = np.union1d(fa, mo)
    leaves = np.setdiff1d(ind, parents)
    founders = ind[(fa == 0) & (mo == 0)]
    inner = np.setdiff1d(np.setdiff1d(ind, leaves), founders)

    def some(pool, k):
        return r.choice(pool, size=min(int(k), len(pool)), replace=False) if len(pool) and k > 0 else np.zeros(0, dtype=np.int64)

    n_pro = int(r.choice([1, 2, 7, 15, 16, 17, 33, 63, 64, 65, 100, 200]))
    pro = np.concatenate([some(leaves, n_pro), some(inner, r.integers(0, 6)), some(founders, r.integers(0, 3))]).astype(np.int64)
    if len(pro) == 0:
        pro = ind[-1:].copy()
    pro = pro[np.sort(np.unique(pro, return_index=True)[1])]                    # (a founder without children is a leaf too)
    G = int(r.choice([1, 1, 2, 3, 7, 9, 16, 32]))
    of = r.integers(-1 if G > 1 or len(pro) > 1 else 0, G, size=len(pro))
    of[int(r.integers(len(pro)))] = int(r.integers(G))                          # somebody is in a group
    groups = None
    if G > 1 or case % 2:
        groups = of.astype(np.int32)
    if case % 2:                                                                # repeats and another order
        extra = r.integers(len(pro), size=int(r.integers(1, 5)))
        order = r.permutation(len(pro) + len(extra))
        pro, groups = np.concatenate([pro, pro[extra]])[order], np.concatenate([groups, groups[extra]])[order]
    S, panel, _ = _sims_and_panel(r, max(1, min(65, ROWS_CAP // n // 128)))
    chunk = int(r.choice([0, 0, 1, 2, 5, 16, 19, 33, 64, 4096]))
    id_map = str(r.choice(ID_MAPS))
    new = _id_map(r, id_map, fa, mo)
    ind, fa, mo, pro = new[ind], new[fa], new[mo], new[pro]
    seed_kind = str(r.choice(SEED_KINDS[1:]))                                   # every seed has a high half
    seed = {"high_half": int(r.integers(1, 1 << 32)) << 32, "top_bit": int(r.integers(1 << 63, 1 << 64, dtype=np.uint64)),
            "all_ones": (1 << 64) - 1}[seed_kind]
    return dict(ind=ind, fa=fa, mo=mo, pro=pro, groups=groups, G=G, S=S, seed=seed, panel=panel, chunk=chunk, by_proband=bool(r.integers(2)), id_map=id_map)


def shape(c, n_labels):
    """(chunks, a ragged last chunk, panels, a ragged last panel) as the rules of csrc/origin.h and csrc/drop_plan.h give them."""
    widest = 639 // c["G"]
    lc = min(n_labels, widest, c["chunk"] if c["chunk"] else widest)
    pn, panels = panel_pairs(c["S"], c["panel"])
    return -(-n_labels // lc), n_labels % lc != 0, panels, -(-c["S"] // 128) % pn != 0


def test_the_cases_reach_what_they_claim():
    from ident_oracle import IdentVector
    chunks = ragged = panels = ragged_panels = one = many = on = off = ungrouped = empty = high = repeats = plain = 0
    maps, sizes = set(), set()
    for case in CASES:
        c = make_case(case)
        again = make_case(case)
        assert all(np.array_equal(c[k], again[k]) for k in c), case                       # a pure function of its number
        assert len(c["ind"]) * c["S"] <= ROWS_CAP and c["seed"] >= 2**32
        groups = np.zeros(len(c["pro"]), dtype=np.int32) if c["groups"] is None else c["groups"]
        assert groups.min() >= -1 and groups.max() < c["G"] and np.any(groups >= 0)
        assert all(len(set(groups[c["pro"] == p].tolist())) == 1 for p in np.unique(c["pro"]).tolist())     # an ID has one group
        o = IdentVector(c["ind"], c["fa"], c["mo"], c["pro"])
        k, rag, p, rag_p = shape(c, o.n_labels)
        chunks += k > 1
        ragged += rag and k > 1
        panels += p > 1
        ragged_panels += rag_p
        one += c["G"] == 1
        many += c["G"] > 8
        on += c["by_proband"]
        off += not c["by_proband"]
        ungrouped += bool(np.any(groups < 0))
        empty += len(np.unique(groups[groups >= 0])) < c["G"]
        plain += c["groups"] is None
        high += c["seed"] >= 2**63
        repeats += len(np.unique(c["pro"])) < len(c["pro"])
        maps.add(c["id_map"])
        sizes.add(c["S"] % 64)
    assert chunks >= 8 and ragged >= 5 and panels >= 5 and ragged_panels >= 3 and one >= 5 and many >= 8 and on >= 10 and off >= 10
    assert ungrouped >= 10 and empty >= 5 and plain >= 2 and high >= 10 and repeats >= 15 and maps == set(ID_MAPS) and len(sizes) >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_random_case(gen, case):
    c = make_case(case)
    args = (c["ind"], c["fa"], c["mo"])
    ref = OriginVector(*args, c["pro"], c["groups"], c["G"], c["S"], c["seed"])
    want = ref.at(c["S"])
    h = gen.OriginsPlan(*args, c["pro"], c["groups"], n_groups=c["G"], simul_no=c["S"], seed=c["seed"], panel_cols=c["panel"], chunk_labels=c["chunk"],
                        by_proband=c["by_proband"])
    try:
        assert np.array_equal(h.alleles(), ref.alleles) and h.seed == c["seed"] and (h.n_grouped, h.n_groups) == (ref.n, c["G"])
        for _ in range(2):
            h.compute()
            got = h.copies_to_host(), h.autozygous_to_host(), h.matches_to_host(), h.by_proband_to_host() if c["by_proband"] else None
            for g, w in zip(got, want):
                assert g is None or (g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)), (case, np.argwhere(g != w)[:5])
        check_invariants(*got, ref.sizes, c["S"], ref.alleles, ref.pro, ref.group)
        st = h.stats()
        k, _, p, _ = shape(c, ref.n_labels)
        assert (st["chunks"], st["panels"]) == (k, p)
    finally:
        h.close()
