"""Random differential stress of the three gene-dropping sweeps on the GPU (not part of the pytest run by itself;
tests/test_drops_random.py runs a short fixed-seed round of it):
    python tests/stress_drops.py [n_cases] [seed]
Random pedigrees x ID maps (small IDs, IDs in [2^40, 2^62), groups that differ only above bit 32, groups that differ only below it) x
seeds with a low half, a high half, both or every bit x proband lists x, per family, the simulations at the word and pair edges, forced and
ragged panels (every lanes-per-row form of the step kernels), chromosomes at the word edges (every lanes-per-simulation form) and the flags;
for each case gen.SimuPlan (sample, state counts, match counts), gen.IdentityPlan (counts, labels) and gen.SharingPlan (sums, labels), or
the public functions gen.simuSample / gen.simuProb / gen.simuIdentity / gen.simuSharing (now and then with a fresh seed), against the
references of tests/simu_oracle.py, tests/ident_oracle.py and tests/link_oracle.py.  No tolerance anywhere: every comparison is
np.array_equal, and every handle is computed twice.  The host plans are compared with the references' too (plan_checks: no GPU needed).
Prints one `FAIL case=... family=... what=...` line per failing comparison with everything needed to replay it
(tests/drop_case.py <case>), and a summary.

The caps below keep the references cheap: counts_of walks n_pro^2 x S entries, sums_of n_pro^2 x S x L, LinkVector copies labels one
locus at a time on every level (levels x L numpy calls) and holds n_ind x 2 x S x L of them."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
os.environ["GENPHI_ENV_HOOKS"] = "1"      # the knob below is an environment hook: read by the library only under this gate

from stress_sweeps import _differs, lanes_per_row      # noqa: E402

MAX_IND = 1500                # individuals of a drawn pedigree (the plane filler of gen.simuIdentity adds at most MAX_FILL more)
MAX_FILL = 130
MAX_SIMS = 8320               # 65 pairs of words: past the 64 lanes of a wave
IDENT_MAX_PRO, IDENT_PAIR_CAP, IDENT_ROWS_CAP = 150, 1_500_000, 3_000_000           # n_pro^2 S; n_ind S
LINK_MAX_PRO, LINK_PAIR_CAP, LINK_ROWS_CAP, LINK_LOOP_CAP = 100, 2_000_000, 1_200_000, 10_000      # n_pro^2 S L; n_ind S L; levels L
FORMS = [1, 2, 4, 8, 16, 32, 64]
LINK_FORMS = [1, 2, 4, 8, 16, 32]
LAST_PAIR = [1, 5, 16, 48, 63, 64, 65, 80, 112, 123, 127, 128]      # the columns of the last pair of words: 16 | S and 64 !| S at 16, 48, 80, 112
ID_MAPS = ["small", "high", "low_shared", "high_shared"]
SEED_KINDS = ["small", "high_half", "top_bit", "all_ones"]
Q_KINDS = ["zero", "one_bit", "0x5555", "32767", "32768", "random"]


# ------------------------------------------------------------------------------------------------------------------ pedigree
def _pedigree(r, case):
    """(kind, father, mother, sex) on the IDs 1 .. n, parents before children: the three kinds of tests/stress_sweeps.py."""
    from genlib_jl_amd import synth
    from random_pedigree import random_pedigree
    u = r.random()
    if u < 0.40:
        kind = "mating"
        n_gen = int(r.integers(3, 16))
        n_pro = int(r.integers(5, 200))
        per = int(r.integers(8, max(9, min(340, (MAX_IND - n_pro) // (n_gen - 1))) + 1))
        skip = int(r.choice([0, 0, 30, 150, 400, 650, 850]))
        ind, fa, mo, sex, _ = synth.random_mating(n_pro + (n_gen - 1) * per, n_pro, n_gen, seed=case, skip_permille=skip)
        if r.random() < 0.5:                                              # one-parent members
            fa, mo = fa.copy(), mo.copy()
            k = np.arange(len(ind))
            mo[(k % int(r.integers(7, 40)) == 5) & (fa != 0)] = 0
            fa[(k % int(r.integers(7, 40)) == 3) & (mo != 0)] = 0
    elif u < 0.82:
        kind = "random"
        n = int(r.choice([12, 30, 30, 60, 120, 400, 900, MAX_IND]))
        pf, p1, ps = float(r.choice([0.01, 0.05, 0.3])), float(r.choice([0.0, 0.1, 0.3])), float(r.choice([0.0, 0.05, 0.15]))
        back = int(r.choice([5, 50, 400, n]))
        ind, fa, mo, sex = random_pedigree(r, n, pf, p1, ps, back, max_depth=int(r.choice([4, 4, 8, 40, 120])))
    else:
        kind = "deep"                                                     # 33 - 52 generations, few sires: full sibs everywhere
        n_gen = int(r.integers(33, 53))
        per = int(r.integers(6, MAX_IND // n_gen + 1))
        ind, fa, mo, sex, _ = synth.deep_inbred(n_gen, per, int(r.integers(2, 5)), seed=case)
        mo = mo.copy()
        mo[(np.arange(len(ind)) // per) % 4 == 2] = 0                     # every fourth generation has no mothers: half-founders
    assert np.array_equal(ind, np.arange(1, len(ind) + 1))
    return kind, np.asarray(fa, dtype=np.int64), np.asarray(mo, dtype=np.int64), np.asarray(sex, dtype=np.int64)


def _depth(fa, mo):
    """1 + the longest ascent, for IDs 1 .. n with parents before children."""
    d = [0] * (len(fa) + 1)
    for i, (f, m) in enumerate(zip(fa.tolist(), mo.tolist())):
        d[i + 1] = 1 + max(d[f], d[m])
    return np.asarray(d[1:], dtype=np.int64)


def _closure(fa, mo, ids):
    """bool per individual: the listed IDs and their ancestors."""
    live = np.zeros(len(fa) + 1, dtype=bool)
    live[np.asarray(ids, dtype=np.int64)] = True
    live[0] = False
    fl, ml = fa.tolist(), mo.tolist()
    for i in range(len(fa), 0, -1):
        if live[i]:
            live[fl[i - 1]] = True
            live[ml[i - 1]] = True
    return live[1:]


def _n_labels(fa, mo, live):
    return int(np.count_nonzero(fa[live] == 0) + np.count_nonzero(mo[live] == 0))


def _filler(fa, mo, sex, delta):
    """Appends a family of its own that carries `delta` >= 2 founder alleles, and returns (father, mother, sex, the ID of its last
    member): delta // 2 founders under a binary tree of their descendants; an odd delta: the root's child by an unknown mother."""
    fa, mo, sex = fa.tolist(), mo.tolist(), sex.tolist()

    def add(f, m):
        fa.append(f)
        mo.append(m)
        sex.append(1 + len(fa) % 2)
        return len(fa)

    tier = [add(0, 0) for _ in range(delta // 2)]
    while len(tier) > 1:
        tier = [add(tier[k], tier[k + 1]) for k in range(0, len(tier) - 1, 2)] + ([tier[-1]] if len(tier) % 2 else [])
    top = add(tier[0], 0) if delta % 2 else tier[0]
    a = lambda x: np.asarray(x, dtype=np.int64)  # noqa: E731
    return a(fa), a(mo), a(sex), top


# ------------------------------------------------------------------------------------------------------------------- ID maps
def _distinct(r, lo, hi, k):
    """k distinct integers of [lo, hi), in a random order."""
    out = np.unique(r.integers(lo, hi, size=k, dtype=np.int64))
    while len(out) < k:
        out = np.unique(np.concatenate([out, r.integers(lo, hi, size=k, dtype=np.int64)]))
    return r.permutation(out)[:k]


def _groups(r, order, keys=None):
    """order cut into groups of 2 .. 8; with keys, a group of two or more ends only where the key changes (or at 8 members): a sibship
    stays together."""
    groups, cur = [], []
    size = int(r.integers(2, 9))
    for pos, x in enumerate(order.tolist()):
        if cur and (len(cur) >= 8 or (len(cur) >= size and (keys is None or keys[pos] != keys[pos - 1]))):
            groups.append(cur)
            cur, size = [], int(r.integers(2, 9))
        cur.append(x)
    groups.append(cur)
    return groups


def full_sibs_sharing_a_low_half(ind, fa, mo):
    """The individuals with both parents known that have a full sib with the same low 32 bits of the ID."""
    both = (fa != 0) & (mo != 0)
    key = np.stack([fa[both], mo[both], ind[both] & 0xFFFFFFFF], axis=1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    return int(np.count_nonzero(cnt[inv.ravel()] >= 2))


def _id_map(r, kind, fa, mo):
    """new ID per old ID 0 .. n (0 stays 0)."""
    n = len(fa)
    new = np.zeros(n + 1, dtype=np.int64)
    if kind == "small":
        new[1:] = np.arange(1, n + 1)
    elif kind == "high":
        new[1:] = _distinct(r, 1 << 40, 1 << 62, n)
    elif kind == "low_shared":                                            # a group: one low half, its members differ only above bit 32
        order = np.lexsort((mo, fa))
        keys = [(int(fa[x]), int(mo[x])) for x in order]
        groups = _groups(r, order, keys)
        lows = _distinct(r, 1, 1 << 32, len(groups))
        for g, lo in zip(groups, lows.tolist()):
            hi = int(r.integers(0, 1 << 29)) + np.arange(len(g), dtype=np.int64) * (2 * int(r.integers(0, 1 << 19)) + 1)
            if r.random() < 0.3:
                hi[0] = 0                                                 # one member below 2^32
            new[np.asarray(g) + 1] = (hi << 32) | lo
    else:                                                                 # a group: one high half, its members differ only below bit 32
        groups = _groups(r, r.permutation(n))
        highs = _distinct(r, 1, 1 << 30, len(groups))
        for g, hi in zip(groups, highs.tolist()):
            lo = (int(r.integers(0, 1 << 32)) + np.arange(len(g), dtype=np.int64) * (2 * int(r.integers(0, 1 << 31)) + 1)) & 0xFFFFFFFF
            new[np.asarray(g) + 1] = (hi << 32) | lo                      # (low halves at and above 2^31 included)
    assert len(np.unique(new[1:])) == n and new[1:].min() > 0
    return new


# ------------------------------------------------------------------------------------------------------- simulations and panels
def _sims_and_panel(r, max_total, weights=(1, 1, 1, 1, 1, 1, 1)):
    """(S, panel argument, pairs of a panel): a lanes-per-row form first (weights: of the forms that fit max_total pairs), then the
    pairs of a panel inside it, then one panel (by default, or forced above S), several whole panels, or several with a ragged last one."""
    forms = [f for f in FORMS if f // 2 + 1 <= max_total]
    w = np.asarray(weights[: len(forms)], dtype=np.float64)
    form = int(r.choice(forms, p=w / w.sum()))
    pn = int(r.integers(form // 2 + 1, min(form if form < 64 else 65, max_total) + 1))
    mode = str(r.choice(["default", "above", "whole", "ragged"], p=[0.3, 0.1, 0.2, 0.4]))
    total, arg = pn, 0
    if mode == "whole" and 2 * pn <= max_total:
        total = pn * int(r.integers(2, min(3, max_total // pn) + 1))
    elif mode == "ragged" and pn >= 2 and pn + 1 <= max_total:
        k = int(r.integers(1, min(3, (max_total - 1) // pn) + 1))
        total = pn * k + int(r.integers(1, min(pn - 1, max_total - pn * k) + 1))
    if total > pn:
        arg = 128 * pn - int(r.choice([0, 1, 100]))
    S = 128 * (total - 1) + int(r.choice(LAST_PAIR))
    if mode == "above":
        arg = S + int(r.choice([0, 1, 100_000]))
    return S, arg, pn


def panel_pairs(S, arg):
    """The pairs of words of a panel and the panels (csrc/drop_plan.h: the argument rounded up to 128 columns and cut to S)."""
    total = (S + 127) // 128
    pn = min(total, (arg + 127) // 128) if arg > 0 else total
    return pn, (total + pn - 1) // pn


def _loci(r, max_loci):
    """L: a lanes-per-simulation form first (1, 2, 4, .. 32 lanes own the pairs of words of a simulation), then the words inside it,
    then a chromosome that fills its last word, enters it by one locus, or ends inside it."""
    forms = [f for f in LINK_FORMS if f == 1 or 128 * (f // 2) + 1 <= max_loci]      # f lanes: more than f / 2 pairs of words
    weight = np.array([1.0, 1.0, 1.0, 2.0, 4.0, 12.0][: len(forms)])                  # few pedigrees leave room for the wide forms
    form = int(r.choice(forms, p=weight / weight.sum()))
    wp = 1 if form == 1 else int(r.integers(form // 2 + 1, form + 1))           # pairs of words
    W = 2 * wp - int(r.integers(0, 2))                                          # an odd W leaves the second word of the last pair empty
    W = max(1, min(W, (max_loci + 63) // 64))
    L = 64 * (W - 1) + int(r.choice([64, 64, 1, 1, 63, int(r.integers(2, 63))]))
    return max(1, min(L, max_loci))


def link_lanes(L):
    wp = ((L + 63) // 64 + 1) // 2
    lanes = 1
    while lanes < wp:
        lanes *= 2
    return lanes


def _blocks_per_side(L, q):
    W = (L + 63) // 64
    first = 8 if q == 0 else ((q & -q).bit_length() - 1) // 2
    return W * (8 - first) + 1


# ---------------------------------------------------------------------------------------------------------------------- case
def make_case(case):
    """Everything of one random case, a pure function of `case`: dict(kind, ind, father, mother, sex, sort, id_map, seed, seed_kind, api,
    fresh_seed, simu, ident, link); the lists of the three families are dicts of their own."""
    from genlib_jl_amd import synth
    r = np.random.default_rng([case, 29])
    kind, fa, mo, sex = _pedigree(r, case)
    n = len(fa)
    ind = np.arange(1, n + 1, dtype=np.int64)
    depth = _depth(fa, mo)
    parents = np.union1d(fa, mo)
    leaves = np.setdiff1d(ind, parents)
    founders = ind[(fa == 0) & (mo == 0)]
    nonleaf = np.setdiff1d(ind, leaves)
    nonfounder = np.setdiff1d(ind, founders)

    def some(pool, k):
        return r.choice(pool, size=min(int(k), len(pool)), replace=False) if len(pool) and k > 0 else np.zeros(0, dtype=np.int64)

    # probands, by the recipe of tests/stress_sweeps.py
    u = r.random() - (0.6 if n <= 30 else 0.3 if n <= 120 else 0.08 if n <= 600 else 0.0)      # everyone: often where all three families' lists hold them
    if u < 0.0:
        pro, pro_kind = (ind.copy() if r.random() < 0.5 else r.permutation(ind)), "everyone"
    elif u < 0.08:
        pro = some(founders, r.integers(1, 12))                           # founders only
        pro, pro_kind = np.concatenate([pro, pro[:1]]), "founders"
    elif u < 0.20:
        pro, pro_kind = some(leaves, r.integers(1, 200)), "leaves"
    else:
        pro = np.concatenate([some(leaves, r.integers(1, 150)), some(nonleaf, r.integers(0, 12)), some(founders, r.integers(0, 5))])
        pro = np.concatenate([pro, r.choice(pro, size=int(r.integers(0, 5)))])
        pro, pro_kind = r.permutation(pro), "mixed"
    pro = np.asarray(pro, dtype=np.int64)
    api = "wrappers" if r.random() < 0.3 else "handles"                   # the public functions take no panel and no all_pairs
    fresh = bool(api == "wrappers" and r.random() < 0.4)

    # ---- simu
    S, arg, _ = _sims_and_panel(r, MAX_SIMS // 128)
    above = _closure(fa, mo, pro)                                         # the probands and their ancestors
    inside = ind[above]
    n_anc = int(r.integers(1, 6)) if r.random() < 0.3 else int(r.integers(6, 60))
    anc = np.concatenate([some(np.intersect1d(founders, inside), r.integers(1, n_anc + 1)), some(np.intersect1d(nonfounder, inside), r.integers(0, n_anc // 2 + 2)),
                          some(ind, r.integers(0, 3))])
    if len(anc) == 0:
        anc = ind[:1].copy()
    if r.random() < 0.5:                                                  # a listed ancestor below another: a child of one, inside
        kids = inside[np.isin(fa[inside - 1], anc) | np.isin(mo[inside - 1], anc)]
        anc = np.concatenate([anc, some(kids, 2)])
    if r.random() < 0.4:
        anc = np.concatenate([anc, pro[:1]])                              # a proband that is a listed ancestor
    _, first = np.unique(anc, return_index=True)
    anc = anc[np.sort(first)].astype(np.int64)                            # distinct: an ancestor listed with two states is an error
    states = r.choice([0, 1, 2], size=len(anc), p=[0.2, 0.45, 0.35]).astype(np.int64)
    if r.random() < 0.5:
        k = np.flatnonzero(np.isin(anc, nonfounder))
        if len(k):
            states[k[0]] = 0                                              # a state-0 blocker below the founders
    if r.random() < 0.15:
        states[:] = 0                                                     # no live row at all
    if r.random() < 0.2:
        anc, states = np.concatenate([anc, anc[:1]]), np.concatenate([states, states[:1]])       # an equal repeat is allowed
    state_pro = [r.integers(0, 3, size=len(pro)) for _ in range(int(r.integers(2, 4)))]
    if r.random() < 0.3:
        state_pro[-1] = np.full(len(pro), int(r.integers(0, 3)))
    simu = dict(pro=pro, anc=anc, states=states, S=S, panel=arg, no_sample=bool(r.random() < 0.3), state_pro=state_pro)

    # ---- ident
    room = max(1, min(MAX_SIMS, IDENT_ROWS_CAP // (n + MAX_FILL)) // 128)
    if pro_kind == "everyone" and len(pro) <= IDENT_MAX_PRO and r.random() < 0.7:
        room = max(1, min(room, IDENT_PAIR_CAP // len(pro) ** 2 // 128))    # few enough simulations to keep everyone
    iS, iarg, _ = _sims_and_panel(r, room, weights=(2, 2, 2, 1, 1, 1.5, 1.5))
    ipro = pro[: max(1, min(IDENT_MAX_PRO, int(np.sqrt(IDENT_PAIR_CAP / iS))))]
    if len(ipro) >= 32 and r.random() < 0.25:
        ipro = ipro[: len(ipro) // 32 * 32]
    if r.random() < 0.55 and pro_kind != "everyone":                      # the allele table at a plane edge: 2^k - 1, 2^k, 2^k + 1 labels
        keep = ipro[:-1] if len(ipro) > 1 and (len(ipro) % 32 == 0 or len(ipro) >= IDENT_MAX_PRO) else ipro      # the filler's proband takes a place
        have = _n_labels(fa, mo, _closure(fa, mo, keep))
        edges = [w for w in sorted({(1 << k) + e for k in range(1, 12) for e in (-1, 0, 1)}) if have + 2 <= w <= have + MAX_FILL]
        if edges:
            want = edges[int(r.integers(0, min(len(edges), 4)))]
            fa, mo, sex, top = _filler(fa, mo, sex, want - have)
            ipro = np.concatenate([keep, [top]])
            n = len(fa)
            ind, depth = np.arange(1, n + 1, dtype=np.int64), _depth(fa, mo)
    ident = dict(pro=ipro, S=iS, panel_cols=iarg, labels=bool(r.random() < 0.6), all_pairs=bool(r.random() < 0.4))

    # ---- link
    lS = int(r.choice([1, 2, 3, 3, 4, 5, 5, 7, 8]))
    lpro = pro[:LINK_MAX_PRO]
    levels = int(depth[_closure(fa, mo, lpro)].max())
    room = max(1, min(4096, LINK_ROWS_CAP // n, LINK_LOOP_CAP // max(levels - 1, 1)))
    keep_all = pro_kind == "everyone" and len(pro) <= LINK_MAX_PRO and r.random() < 0.7
    if keep_all:
        room = max(1, min(room, LINK_PAIR_CAP // len(pro) ** 2))           # a chromosome short enough to keep everyone
    L = _loci(r, room)
    lS = max(1, min(lS, LINK_ROWS_CAP // (n * L), LINK_PAIR_CAP // (len(pro) ** 2 * L) if keep_all else lS))      # the chromosome first, then the simulations that still fit
    lpro = lpro[: max(1, int(np.sqrt(LINK_PAIR_CAP / (lS * L))))]
    q_kind = str(r.choice(Q_KINDS))
    q = {"zero": 0, "one_bit": 1 << int(r.integers(0, 15)), "0x5555": 0x5555, "32767": 32767, "32768": 32768, "random": int(r.integers(1, 32768))}[q_kind]
    link = dict(pro=lpro, L=L, q=q, q_kind=q_kind, S=lS, panel_sims=int(r.choice([0, 1, 2, 2, 3, 3, 5, lS, 1000])), labels=bool(r.random() < 0.6),
                all_pairs=bool(r.random() < 0.4))
    if api == "wrappers":
        ident.update(panel_cols=0, all_pairs=False)
        link.update(panel_sims=0, all_pairs=False)

    # ---- file order, IDs and the seed
    sort = bool(r.random() < 0.5)
    if not sort:
        ind, fa, mo, sex = synth.parents_first_shuffle(ind, fa, mo, sex, seed=case & 0xffff)
    elif r.random() < 0.8:                                                # any file order: the rank order is another
        o = r.permutation(n)
        ind, fa, mo, sex = ind[o], fa[o], mo[o], sex[o]
    id_map = str(r.choice(ID_MAPS))
    new = _id_map(r, id_map, fa[np.argsort(ind)], mo[np.argsort(ind)])
    if id_map == "low_shared" and full_sibs_sharing_a_low_half(new[ind], new[fa], new[mo]) == 0:
        id_map = "high"                                                   # a pedigree without full sibs
        new = _id_map(r, id_map, fa, mo)
    ind, fa, mo = new[ind], new[fa], new[mo]
    for fam in (simu, ident, link):
        fam["pro"] = new[fam["pro"]]
    simu["anc"] = new[simu["anc"]]
    seed_kind = str(r.choice(SEED_KINDS))
    seed = {"small": int(r.integers(1, 3000)), "high_half": int(r.integers(1, 1 << 32)) << 32,
            "top_bit": int(r.integers(1 << 63, 1 << 64, dtype=np.uint64)), "all_ones": (1 << 64) - 1}[seed_kind]
    return dict(kind=kind, ind=ind, father=fa, mother=mo, sex=sex, sort=sort, id_map=id_map, seed=seed, seed_kind=seed_kind, api=api,
                fresh_seed=fresh, pro_kind=pro_kind, simu=simu, ident=ident, link=link)


def describe(c):
    s, i, k = c["simu"], c["ident"], c["link"]
    return ("kind=%s n_ind=%d sort=%s ids=%s seed=%#x (%s) api=%s%s pro=%s | simu: n_pro=%d n_anc=%d S=%d panel=%s no_sample=%s | "
            "ident: n_pro=%d S=%d panel_cols=%d labels=%s all_pairs=%s | link: n_pro=%d L=%d q=%d S=%d panel_sims=%d labels=%s all_pairs=%s" % (
                c["kind"], len(c["ind"]), c["sort"], c["id_map"], c["seed"], c["seed_kind"], c["api"], " fresh seed" if c["fresh_seed"] else "",
                c["pro_kind"], len(s["pro"]), len(s["anc"]), s["S"], s["panel"] or None, s["no_sample"], len(i["pro"]), i["S"], i["panel_cols"],
                i["labels"], i["all_pairs"], len(k["pro"]), k["L"], k["q"], k["S"], k["panel_sims"], k["labels"], k["all_pairs"]))


# -------------------------------------------------------------------------------------------------------- handles and plans
def genealogy(c, gen):
    return gen.genealogy({"ind": c["ind"], "father": c["father"], "mother": c["mother"], "sex": c["sex"]}, sort=c["sort"])


def handles(c, gen, args, seed=None):
    """(SimuPlan, IdentityPlan, SharingPlan) of a case on the pedigree arrays in rank order; nothing is computed."""
    s, i, k = c["simu"], c["ident"], c["link"]
    seed = c["seed"] if seed is None else seed
    os.environ.pop("GENPHI_SIMU_PANEL", None)
    if s["panel"]:
        os.environ["GENPHI_SIMU_PANEL"] = str(s["panel"])
    try:
        hs = gen.SimuPlan(*args, s["pro"], s["anc"], s["states"], simul_no=s["S"], seed=seed, no_sample=s["no_sample"])
    finally:
        os.environ.pop("GENPHI_SIMU_PANEL", None)
    hi = gen.IdentityPlan(*args, i["pro"], simul_no=i["S"], seed=seed, labels=i["labels"], panel_cols=i["panel_cols"], all_pairs=i["all_pairs"])
    hl = gen.SharingPlan(*args, k["pro"], loci=k["L"], q=k["q"], simul_no=k["S"], seed=seed, labels=k["labels"], panel_sims=k["panel_sims"],
                         all_pairs=k["all_pairs"])
    return hs, hi, hl


def references(c, args):
    """The three references of a case (the plans only: no simulation yet)."""
    from ident_oracle import IdentVector
    from link_oracle import LinkVector
    from simu_oracle import SimuVector
    s = c["simu"]
    return SimuVector(*args, s["pro"], s["anc"], s["states"]), IdentVector(*args, c["ident"]["pro"]), LinkVector(*args, c["link"]["pro"])


def plan_checks(c, args, hs, hi, hl, os_, oi, ol):
    """(family, name, got, want) of every host-side comparison: the live sets, their levels, the planned rows and the allele tables."""
    one = lambda v: np.array([v], dtype=np.int64)  # noqa: E731
    out = [("simu", "n_live", one(hs.n_live), one(os_.n_live)), ("simu", "levels", one(hs.levels), one(os_.levels)),
           ("simu", "rows_per_level", hs.rows_per_level(), os_.rows_per_level)]
    r = hs.rows()
    ind = np.asarray(args[0])
    order = np.argsort(ind, kind="stable")
    at = order[np.searchsorted(ind[order], r["ids"])] if len(r["ids"]) else np.zeros(0, dtype=np.int64)
    out.append(("simu", "rows: the live set", np.sort(at), np.flatnonzero(os_.level >= 0)))
    out.append(("simu", "rows: ordered by level", one(int(np.all(np.diff(os_.level[at]) >= 0))), one(1)))
    row_of = np.full(len(ind), -1, dtype=np.int64)
    row_of[at] = np.arange(len(at))
    for name, parent in (("father_rows", os_.fa), ("mother_rows", os_.mo)):
        q = parent[at]
        out.append(("simu", "rows: " + name, r[name].astype(np.int64), np.where((q >= 0) & (os_.level[at] > 0), row_of[np.maximum(q, 0)], -1)))
    out.append(("simu", "rows: pro_positions", r["pro_positions"], np.where(os_.state[os_.pro] >= 0, -2 - os_.state[os_.pro], row_of[os_.pro])))
    for fam, h, o in (("ident", hi, oi), ("link", hl, ol)):
        out += [(fam, "n_live", one(h.n_live), one(o.n_live)), (fam, "levels", one(h.levels), one(o.levels)),
                (fam, "rows_per_level", h.rows_per_level(), o.rows_per_level), (fam, "alleles", h.alleles(), o.alleles),
                (fam, "n_labels", one(h.n_labels), one(o.n_labels)), (fam, "planes", one(h.planes), one(o.planes))]
    return out


def classes(c, hs, hi, hl, os_, oi, ol):
    """The classes of tests/test_drops_random.py that a case belongs to, from the case, the handles' host accessors and the references'
    plans."""
    s, i, k = c["simu"], c["ident"], c["link"]
    out = {"sort=%s" % c["sort"], "ids " + c["id_map"], "pro " + c["pro_kind"], "api " + c["api"]}
    if c["fresh_seed"]:
        out.add("fresh seed")
    else:
        out.add("seed " + c["seed_kind"])
    # simu
    pn, panels = panel_pairs(s["S"], s["panel"])
    total = (s["S"] + 127) // 128
    out.add("simu lanes %d" % lanes_per_row(pn))
    out.add("simu one panel" if panels == 1 else "simu several panels")
    if panels > 1 and total % pn:
        out.add("simu ragged last panel")
    if s["S"] % 64:
        out.add("simu S % 64 != 0")
    if s["S"] % 16 == 0 and s["S"] % 64:
        out.add("simu S % 16 == 0, S % 64 != 0")
    if s["no_sample"]:
        out.add("simu no_sample")
    if np.any((os_.level[os_.pro] < 0) & (os_.state[os_.pro] < 0)):
        out.add("simu proband outside the live set")
    if np.any(os_.state[os_.pro] >= 0):
        out.add("simu proband that is a listed ancestor")
    if os_.n_live == 0:
        out.add("simu no live row")
    stepped = os_.level > 0
    if np.any(stepped & (os_.fa >= 0) & (os_.fa == os_.mo)):
        out.add("simu selfing")
    if np.any(stepped & ((os_.fa < 0) != (os_.mo < 0))):
        out.add("simu half-founder")
    if os_.levels >= 30:
        out.add("simu 30 levels")
    if len(np.unique(s["pro"])) < len(s["pro"]):
        out.add("simu repeated probands")
    if len(np.unique(s["pro"])) == len(c["ind"]):
        out.add("simu everyone a proband")
    # ident
    pn, panels = panel_pairs(i["S"], i["panel_cols"])
    out.add("ident lanes %d" % lanes_per_row(pn))
    out.add("ident one panel" if panels == 1 else "ident several panels")
    if panels > 1 and ((i["S"] + 127) // 128) % pn:
        out.add("ident ragged last panel")
    n = len(i["pro"])
    out.add("ident n_pro <= 32" if n <= 32 else "ident n_pro 33 .. 64" if n <= 64 else "ident n_pro > 64")
    if n % 32 == 0:
        out.add("ident n_pro % 32 == 0")
    if i["all_pairs"]:
        out.add("ident all_pairs")
    if not i["labels"]:
        out.add("ident labels off")
    for e, name in ((0, "at"), (-1, "below"), (1, "above")):
        nl = oi.n_labels - e
        if nl >= 2 and nl & (nl - 1) == 0:
            out.add("ident n_labels %s a power of two" % name)
    # link
    W = (k["L"] + 63) // 64
    out.add("link lanes %d" % link_lanes(k["L"]))
    if W % 2:
        out.add("link odd W")
    if k["L"] % 64 == 0:
        out.add("link L % 64 == 0")
    if k["L"] % 64 == 1:
        out.add("link L % 64 == 1")
    if k["q"] == 0:
        out.add("link q = 0")
    if k["q"] == 32768:
        out.add("link q = 32768")
    if bin(k["q"]).count("1") >= 2:
        out.add("link q with several bits")
    ps = min(k["S"], k["panel_sims"]) if k["panel_sims"] else k["S"]
    if ps < k["S"] and k["S"] % ps:
        out.add("link several panels, ragged last")
    if len(k["pro"]) > 32:
        out.add("link n_pro > 32")
    for fam, o, p in (("ident", oi, i["pro"]), ("link", ol, k["pro"])):
        lf, lm = o.fa[o.live], o.mo[o.live]
        if np.any((lf >= 0) & (lf == lm)):
            out.add(fam + " selfing")
        if np.any((lf < 0) != (lm < 0)):
            out.add(fam + " half-founder")
        if o.levels >= 30:
            out.add(fam + " 30 levels")
        if len(np.unique(p)) < len(p):
            out.add(fam + " repeated probands")
        if len(np.unique(p)) == len(c["ind"]):
            out.add(fam + " everyone a proband")
    # what the handles say about the shapes derived above (host only)
    st = hi.stats()
    pn, panels = panel_pairs(i["S"], i["panel_cols"])
    assert (st["panel_cols"], st["panels"], st["lanes_per_row"]) == (128 * pn, panels, lanes_per_row(pn)), st
    st = hl.stats()
    assert (st["panel_sims"], st["panels"], st["lanes_per_sim"]) == (ps, (k["S"] + ps - 1) // ps, link_lanes(k["L"])), st
    return out


# ----------------------------------------------------------------------------------------------------------------------- run
ORACLE_CPU = [0.0]


def _timed(f, *a):
    t = time.process_time()
    try:
        return f(*a)
    finally:
        ORACLE_CPU[0] += time.process_time() - t


def run_case(case, gen, report=None):
    """One case end to end.  Returns (the comparisons that failed as (family, what), the case).  report: a function that gets one
    line per comparison (tests/drop_case.py)."""
    from ident_oracle import counts_of
    from link_oracle import sums_of
    from simu_oracle import match_counts, state_counts
    c = make_case(case)
    what = []

    def check(fam, name, got, want):
        d = _differs(got, want)
        if report:
            report("  %-6s %-44s %s" % (fam, name, "ok" if d is None else d))
        if d is not None:
            what.append((fam, name))

    def failed(fam, e):
        what.append((fam, "exception %s: %s" % (type(e).__name__, e)))
        if report:
            report("  %-6s %s" % (fam, what[-1][1]))

    s, i, k = c["simu"], c["ident"], c["link"]
    hs = hi = hl = None
    try:
        ped = genealogy(c, gen)
        args = (ped.ind, ped.father, ped.mother)
        os_, oi, ol = _timed(references, c, args)
        hs, hi, hl = handles(c, gen, args)
        for fam, name, got, want in plan_checks(c, args, hs, hi, hl, os_, oi, ol):
            check(fam, name, got, want)
    except Exception as e:          # noqa: BLE001
        failed("plan", e)
        for h in (hs, hi, hl):
            if h is not None:
                h.close()
        return what, c
    wrappers, seed = c["api"] == "wrappers", (None if c["fresh_seed"] else c["seed"])

    # ---- simu
    try:
        if wrappers:
            os.environ.pop("GENPHI_SIMU_PANEL", None)
            if s["panel"]:
                os.environ["GENPHI_SIMU_PANEL"] = str(s["panel"])
            probs = [gen.simuProb(ped, s["pro"], sp, s["anc"], s["states"], simulNo=s["S"], seed=seed) for sp in s["state_pro"]]
            for sp, p in zip(s["state_pro"], probs):
                want = _timed(os_.sample, s["S"], p.seed)
                if seed is not None:
                    check("simu", "simuProb seed", np.array([p.seed], dtype=np.uint64), np.array([seed], dtype=np.uint64))
                check("simu", "simuProb marginal", p.marginal, state_counts(want)[np.arange(len(sp)), sp] / float(s["S"]))
                check("simu", "simuProb by_number", p.by_number, np.bincount(match_counts(want, sp), minlength=len(sp) + 1) / float(s["S"]))
                check("simu", "simuProb joint", np.array([p.joint]), np.array([float(np.count_nonzero(match_counts(want, sp) == len(sp)) / float(s["S"]))]))
            if seed is not None:
                check("simu", "simuSample", gen.simuSample(ped, s["pro"], s["anc"], s["states"], simulNo=s["S"], seed=seed), want)
        else:
            want = _timed(os_.sample, s["S"], seed)
            pn, panels = panel_pairs(s["S"], s["panel"])
            for again in ("", " (second compute)"):
                hs.compute()
                if s["no_sample"]:
                    try:
                        hs.sample_to_host()
                        what.append(("simu", "sample_to_host under no_sample did not raise"))
                    except ValueError:
                        pass
                else:
                    check("simu", "sample" + again, hs.sample_to_host(), want)
                check("simu", "state_counts" + again, hs.state_counts(), state_counts(want))
                for j, sp in enumerate(s["state_pro"]):
                    for ask in ("", ", asked again"):
                        check("simu", "match_counts %d%s%s" % (j, ask, again), hs.match_counts(sp), match_counts(want, sp))
                check("simu", "state_counts after match_counts" + again, hs.state_counts(), state_counts(want))
            st = hs.stats()
            check("simu", "stats: panel_cols, panels, lanes_per_row", np.array([st["panel_cols"], st["panels"], st["lanes_per_row"]]),
                  np.array([128 * pn, panels, lanes_per_row(pn)]))
    except Exception as e:          # noqa: BLE001
        failed("simu", e)
    finally:
        os.environ.pop("GENPHI_SIMU_PANEL", None)
        hs.close()

    # ---- ident
    try:
        n = len(i["pro"])
        if wrappers:
            res = gen.simuIdentity(ped, i["pro"], simulNo=i["S"], seed=seed, labels=i["labels"])
            want = _timed(oi.labels, i["S"], res.seed)
            check("ident", "simuIdentity counts", res.counts, _timed(counts_of, want))
            check("ident", "simuIdentity alleles", res.alleles, oi.alleles)
            if i["labels"]:
                check("ident", "simuIdentity labels", res.labels, want)
        else:
            want = _timed(oi.labels, i["S"], seed)
            counts = _timed(counts_of, want)
            for again in ("", " (second compute)"):
                hi.compute()
                check("ident", "counts" + again, hi.counts_to_host(), counts)
                if i["labels"]:
                    check("ident", "labels" + again, hi.labels_to_host(), want)
            st = hi.stats()
            pairs = n * n if i["all_pairs"] else n * (n + 1) // 2
            check("ident", "stats: word_ops", np.array([st["word_ops"]]), np.array([float(pairs * ((i["S"] + 63) // 64) * (12 * oi.planes + 40))]))
    except Exception as e:          # noqa: BLE001
        failed("ident", e)
    finally:
        hi.close()

    # ---- link
    try:
        n, L, q, S = len(k["pro"]), k["L"], k["q"], k["S"]
        if wrappers:
            res = gen.simuSharing(ped, k["pro"], loci=L, probRecomb=q / 65536.0, simulNo=S, seed=seed, labels=k["labels"])
            want = _timed(ol.labels, S, L, q, res.seed)
            check("link", "simuSharing q", np.array([res.q]), np.array([q]))
            check("link", "simuSharing sums", res.sums, _timed(sums_of, want))
            check("link", "simuSharing alleles", res.alleles, ol.alleles)
            if k["labels"]:
                check("link", "simuSharing labels", res.labels, want)
        else:
            want = _timed(ol.labels, S, L, q, seed)
            sums = _timed(sums_of, want)
            for again in ("", " (second compute)"):
                hl.compute()
                got = hl.sums_to_host()
                check("link", "sums" + again, got, sums)
                if k["labels"]:
                    mine = hl.labels_to_host()
                    check("link", "labels" + again, mine, want)
                    check("link", "sums against sums_of(its own labels)" + again, got, sums if np.array_equal(mine, want) else _timed(sums_of, mine))
            st = hl.stats()
            W = (L + 63) // 64
            pairs = n * n if k["all_pairs"] else n * (n + 1) // 2
            known = 2 * ol.n_live - ol.n_labels
            check("link", "stats: word_ops, philox_blocks, bytes", np.array([st["word_ops"], st["philox_blocks"], st["algorithmic_bytes"]]),
                  np.array([float(pairs * S * W * (8 * ol.planes + 32)), float(known * S * _blocks_per_side(L, q)),
                            float(48 * ol.planes * known * S * ((W + 1) // 2))]))
            check("link", "stats: lanes_per_sim, planes, levels", np.array([st["lanes_per_sim"], st["planes"], st["levels"]]),
                  np.array([link_lanes(L), ol.planes, ol.levels]))
    except Exception as e:          # noqa: BLE001
        failed("link", e)
    finally:
        hl.close()
    return what, c


def main():
    import genlib_jl_amd as gen
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 12345
    rng = np.random.default_rng(seed0)
    t0, n_fail = time.time(), 0
    for k in range(n_cases):
        case = int(rng.integers(1 << 30))
        what, c = run_case(case, gen)
        if what:
            n_fail += 1
            for fam, name in what:
                print("FAIL case=%d family=%s what=%s | %s" % (case, fam, name, describe(c)), flush=True)
        if (k + 1) % 20 == 0:
            print("... %d cases, %d failures, %.0f s" % (k + 1, n_fail, time.time() - t0), flush=True)
    print("the references took %.1f s of CPU" % ORACLE_CPU[0], flush=True)
    print("drop stress: %d cases, %d failures in %.0f s (seed %d)" % (n_cases, n_fail, time.time() - t0, seed0), flush=True)
    return 1 if n_fail else 0


def round_cases(n_cases, seed0):
    """The case numbers of `python tests/stress_drops.py n_cases seed0`."""
    rng = np.random.default_rng(seed0)
    return [int(rng.integers(1 << 30)) for _ in range(n_cases)]


if __name__ == "__main__":
    sys.exit(main())
