"""Pedigrees whose gen.sparse_phi waves have chosen widths (test infrastructure, imported by the sparse_phi tests).

gen.sparse_phi (csrc/sparse_phi.hip) runs one wave per depth and picks a wave's kernels by the size of its old set n_old: the live
individuals the new rows read.  wide_waves() builds discrete generations of given sizes in which generation g is exactly wave g,
so the widths of the waves are a test's choice; n_old() reads them back from the schedule the product will follow
(_capi.sparse_schedule), which is what a test asserts before it relies on a regime.
"""
import numpy as np


def wide_waves(widths, early_probands=None, one_parent_every=0, skip_permille=0, window=48, cross_permille=20, seed=1):
    """Generation g has widths[g] members (generation 0: founders); IDs 1.. in generation order.

    - Every member of generation g-1 is a parent: child c of generation g gets the members p of g-1 with
      p * widths[g] // widths[g-1] == c (at most two, since widths[g] >= ceil(widths[g-1] / 2) is required).
    - The missing parents are random: near the child's position in g-1 (+- `window`), or with `cross_permille`
      anywhere in g-1, so half-sibs, cousins and inbreeding give non-trivial kinships (a funnel of disjoint couples would
      be all zeros off the diagonal).  Near positions keep the live set of the reference's queue close to the wider of two
      neighbouring generations: a parent retires about where its children are processed.
    - With `skip_permille` a random parent comes from g-2 instead (never both parents: the child stays at depth g); that
      parent survives wave g-1 ("dragged" into wave g's old set).
    - With `one_parent_every` = k, every k-th child without two covering parents keeps one parent only.
    - Probands: the last generation, plus early_probands[g] members of each earlier generation g (evenly spaced), which
      survive every later wave.  Adding early probands does not change the parents: n_old of every wave from g + 3 on
      grows by exactly early_probands[g].

    Returns (ind, father, mother, sex, pro)."""
    widths = [int(w) for w in widths]
    for g in range(1, len(widths)):
        if 2 * widths[g] < widths[g - 1]:
            raise ValueError(f"generation {g}: {widths[g]} members cannot have every one of {widths[g - 1]} parents")
    rng = np.random.default_rng(seed)
    starts = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    n = int(starts[-1])
    father = np.zeros(n, np.int64)
    mother = np.zeros(n, np.int64)
    for g in range(1, len(widths)):
        w, prev = widths[g], widths[g - 1]
        par = np.full((w, 2), -1, np.int64)                       # positions in g-1 (or g-2: position + a flag below)
        cover = np.arange(prev, dtype=np.int64) * w // prev
        first = np.ones(prev, bool)
        first[1:] = cover[1:] != cover[:-1]
        par[cover[first], 0] = np.flatnonzero(first)
        par[cover[~first], 1] = np.flatnonzero(~first)
        anchor = np.arange(w, dtype=np.int64) * prev // w
        near = np.clip(anchor[:, None] + rng.integers(-window, window + 1, (w, 2)), 0, prev - 1)
        far = rng.integers(0, prev, (w, 2))
        pick = np.where(rng.integers(0, 1000, (w, 2)) < cross_permille, far, near)
        from2 = np.zeros((w, 2), bool)
        if g >= 2 and skip_permille > 0:
            pp = widths[g - 2]
            from2[:, 1] = rng.integers(0, 1000, w) < skip_permille
            pick[from2[:, 1], 1] = np.clip(anchor[from2[:, 1]] * pp // prev + rng.integers(-window, window + 1, int(from2[:, 1].sum())), 0, pp - 1)
        for k in (0, 1):                                           # a random parent where no covering one is
            m = par[:, k] < 0
            par[m, k] = pick[m, k]
            from2[~m, k] = False
        same = (par[:, 0] == par[:, 1]) & ~from2[:, 1] & ~from2[:, 0]
        par[same, 1] = (par[same, 1] + 1) % prev                    # (never one individual as both parents)
        if prev == 1:
            par[:, 1] = -2
        pid = np.where(from2, starts[g - 2] if g >= 2 else 0, starts[g - 1]) + par + 1
        pid[par == -2] = 0
        if one_parent_every:
            covered2 = (cover[~first]).tolist()
            drop = np.zeros(w, bool)
            drop[one_parent_every - 1::one_parent_every] = True
            drop[covered2] = False
            pid[drop, 1] = 0
        lo, hi = int(starts[g]), int(starts[g + 1])
        father[lo:hi] = pid[:, 0]
        mother[lo:hi] = pid[:, 1]
    ind = np.arange(1, n + 1, dtype=np.int64)
    sex = (np.arange(n) % 2 + 1).astype(np.int64)
    pro = [ind[starts[-2]:]]
    for g, k in enumerate(early_probands or []):
        if k and g < len(widths) - 1:
            pro.append(ind[starts[g] + np.linspace(0, widths[g] - 1, int(k)).astype(np.int64)])
    return ind, father, mother, sex, np.concatenate(pro[1:] + pro[:1])


def waves(order, retire_at, wave):
    """(n_old, n_new) per wave of the sweep gen.sparse_phi runs, from _capi.sparse_schedule's (order, retire_at, wave):
    n_old(w) = #{u : wave(u) < w and (retire_at(u) < 0 or retire_at(u) >= first processing index of wave w)}."""
    wave = np.asarray(wave, np.int64)
    retire_at = np.asarray(retire_at, np.int64)
    nw = int(wave.max()) + 1 if len(wave) else 0
    n_new = np.bincount(wave, minlength=nw)
    first = np.concatenate([[0], np.cumsum(n_new)[:-1]])
    # u is in the old set of waves wave(u)+1 .. last, last = the last wave that starts at or before retire_at(u)
    last = np.where(retire_at < 0, nw - 1, np.searchsorted(first, retire_at, side="right") - 1)
    diff = np.zeros(nw + 1, np.int64)
    live = last >= wave + 1
    np.add.at(diff, wave[live] + 1, 1)
    np.add.at(diff, last[live] + 1, -1)
    return np.cumsum(diff)[:nw], n_new


def n_old_of(gen, ind, father, mother, sex, pro, sort=True):
    """(n_old, n_new) per wave of gen.sparse_phi(genealogy(...; sort), pro), from the host-only schedule."""
    from genlib_jl_amd import _capi
    ped = gen.genealogy({"ind": ind, "father": father, "mother": mother, "sex": sex}, sort=sort)
    return waves(*_capi.sparse_schedule(ped.ind, ped.father, ped.mother, pro))


# The largest old set whose T row fits the fused kernel's LDS: 36,864 floats = 144 KB (kFusedMaxOld, csrc/sparse_phi.hip).  Up to
# 12,288 (48 KB) no attribute call is needed; above kFusedMaxOld a wave takes the two-kernel form with T in HBM.
FUSED_MAX_OLD = 36864
DEFAULT_LDS_OLD = 12288

_TWO_KERNEL = [6000, 12000, 24000, 35700, 38000, 21000, 12000, 7000, 4000, 2400, 1500]
CASES = {
    # fused waves at n_old = 12,288 | 12,289 | 20,002 | 24,003 | 36,864 (LDS 48 KB, just above, 2 and 3 mod 4, 144 KB); 12 early
    # probands survive every wave from the third on
    "fused_lds_edges": dict(widths=[8000, 12284, 12281, 19990, 23991, 36852, 20000, 12000, 7000, 4000, 2400, 1500],
                            early_probands=[4, 4, 4], seed=1),
    # the first automatic two-kernel waves: n_old = 36,865, then 38,204 with 21,000 new rows; 3 % of the parents two generations up
    # (dragged survivors); 66 of the 70 early probands of generation 0 top n_old up to exactly 36,865
    "two_kernel_skip": dict(widths=_TWO_KERNEL, early_probands=[70, 4, 4], skip_permille=30, seed=2),
    # the same widths with one-parent members instead of skipped generations
    "two_kernel_one_parent": dict(widths=_TWO_KERNEL[:3] + [36853] + _TWO_KERNEL[4:], early_probands=[4, 4, 4], one_parent_every=5, seed=3),
    # two_kernel_skip in a parents-first shuffled file order, genealogy(...; sort=false), 112 more ancestors among the probands
    "two_kernel_unsorted": dict(widths=_TWO_KERNEL, early_probands=[70, 4, 4], skip_permille=30, seed=2, shuffle=5),
    # the proband block's ways to the host: the pinned staging buffer holds up to 8,192 probands (256 MB), beyond is a plain 2D copy
    "copy_small": dict(widths=[50, 80, 100], early_probands=[3], seed=4),
    "copy_8192": dict(widths=[1500, 3000, 6000, 8192], seed=5),
    "copy_8193": dict(widths=[1500, 3000, 6000, 8193], seed=6),
    # 4,201 waves: no per-wave timing events beyond 4,096 waves
    "many_waves": dict(widths=[6] + [5, 4, 6, 5] * 1050, early_probands=[1, 1], seed=7),
}


def case(name):
    """(ind, father, mother, sex, pro, sort) of CASES[name]."""
    kw = dict(CASES[name])
    shuffle = kw.pop("shuffle", None)
    ind, fa, mo, sex, pro = wide_waves(**kw)
    if shuffle is None:
        return ind, fa, mo, sex, pro, True
    from genlib_jl_amd import synth
    i2, f2, m2, s2 = synth.parents_first_shuffle(ind, fa, mo, sex, seed=shuffle)
    # ancestors among the probands: members of the first three generations (ancestors of everyone) and of the two-kernel waves
    # (generations 4 and 5: their outliving entries with later members of the same wave come from the new x new kernel)
    top, wide = sum(kw["widths"][:3]), sum(kw["widths"][:4])
    rng = np.random.default_rng(shuffle)
    extra = np.unique(np.concatenate([rng.integers(1, top + 1, 48), rng.integers(wide + 1, sum(kw["widths"][:6]) + 1, 64)]))
    return i2, f2, m2, s2, np.concatenate([pro, extra[~np.isin(extra, pro)]]), False


def check_regime(gen, name, ind, fa, mo, sex, pro, sort):
    """Asserts, from the schedule gen.sparse_phi will follow, that CASES[name] reaches the path it is there for; returns (n_old, n_new)."""
    from genlib_jl_amd import _capi
    ped = gen.genealogy({"ind": ind, "father": fa, "mother": mo, "sex": sex}, sort=sort)
    order, retire_at, wave = _capi.sparse_schedule(ped.ind, ped.father, ped.mother, pro)
    n_old, n_new = waves(order, retire_at, wave)
    busy = n_new > 0
    fused, two = busy & (n_old <= FUSED_MAX_OLD), busy & (n_old > FUSED_MAX_OLD)
    n_pro = len(set(np.asarray(pro).tolist()))
    # (survivors of a wave: old members still live after it; early probands make them in every wave from the third on)
    first = np.concatenate([[0], np.cumsum(n_new)[:-1]])
    if name == "fused_lds_edges":
        assert not two.any() and fused.all()
        assert {12288, 12289, 36864} <= set(n_old.tolist()), n_old
        mid = n_old[(n_old > 16384) & (n_old < FUSED_MAX_OLD)]
        assert {1, 2, 3} <= set((n_old[n_old > DEFAULT_LDS_OLD] % 4).tolist()) and len(mid), n_old
        big = n_old > DEFAULT_LDS_OLD
        assert (n_old[big] - np.asarray(CASES[name]["widths"])[np.flatnonzero(big) - 1] > 0).all()     # survivors in every wide wave
    elif name.startswith("two_kernel"):
        if name != "two_kernel_unsorted":
            assert 36865 in n_old.tolist(), n_old
        assert (two & (n_new >= 20000)).any() and fused.sum() >= 5, (n_old, n_new)
        assert n_old[two].max() <= 40000
        if "skip" in name or "unsorted" in name:                 # dragged: non-probands of wave w-2 in the old set of a two-kernel wave
            w = np.asarray(wave, np.int64)
            dragged = [int(((w == k - 2) & (retire_at >= first[k])).sum()) for k in np.flatnonzero(two)]
            assert min(dragged) > 0, dragged
        if "one_parent" in name:
            assert (np.asarray(mo) == 0).sum() > len(CASES[name]["widths"]) * 1000
    elif name.startswith("copy_"):
        assert n_pro == {"copy_small": 103, "copy_8192": 8192, "copy_8193": 8193}[name] and fused.all()
    elif name == "many_waves":
        assert len(n_new) > 4096
    return n_old, n_new
