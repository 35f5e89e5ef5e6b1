"""genlib.jl_amd -- MI355X-native drop-in for GenLib.jl's dense kinship matrix `gen.phi`.

Host-side mirror of the reference interface for this ONE path (the reference's host
language, Julia, is not available in the build image; the Julia shim that a GenLib.jl
maintainer would add is in julia/GenLibAMD.jl and INTEGRATION.md).  Same names, argument
meaning, printed lines and error behaviour as the reference:

    import genlib_jl_amd as gen            # loader shim at the repo root
    ped = gen.genealogy(gen.geneaJi)       # src/create.jl:161-189 (+ depth sort :196-254)
    gen.pro(ped); gen.founder(ped)         # src/identify.jl:35-39, :15-19
    phi = gen.phi(ped, verbose=True)       # src/compute.jl:233-304 -> float32 (N, N)
    gen.phi(ped[1], ped[2])                # src/compute.jl:66-95: pairwise, Float64 (one Float64 GPU sweep)
    gen.phiMean(phi)                       # src/compute.jl:454-459 (PhiPlan.phi_mean(): on the device)
    K = gen.sparse_phi(ped); K[1, 2]       # src/compute.jl:321-447, :31-46; gen.phiMean(K) :467-472
    gen.f(ped, [1])                        # src/compute.jl:500-511, from one Float64 GPU sweep over the parents
    gen.branching(ped, pro=[1])            # src/extract.jl:65-186, native pruning (csrc/loader.cpp)
    gen.gc(ped)                            # src/compute.jl:518-595: genetic contributions (csrc/gc.hip)
    gen.occ(ped); gen.rec(ped)             # src/describe.jl:184-238, :133-145: occurrences, coverage (csrc/occ.hip)
    gen.findMRCA(ped, [1, 2, 29])          # src/identify.jl:83-160: MRCAs and meioses; gen.meioses, gen.findDistance,
                                           # gen.findFounders, gen.ancestor (csrc/dist.hip + csrc/loader.cpp)
    gen.depths(ped)                        # src/describe.jl:241-279 reduced: paths, shortest, longest and mean ascent per pair
                                           # (csrc/depth.hip); gen.genMin, gen.genMax, gen.genMean: GENLIB's gen.min / gen.max / gen.mean
    gen.completeness(ped); gen.depth(ped)  # src/describe.jl:73-125, :43-66: ascents by generation (csrc/completeness.hip);
                                           # gen.nomen, gen.nowomen, gen.noind, ped.show() (src/describe.jl:6-36, src/create.jl:76-111)
    gen.implex(ped)                        # GENLIB's gen.implex: distinct ancestors by generation (csrc/implex.hip)
    gen.simuSample(ped); gen.simuProb(..)  # GENLIB's gene dropping: marked alleles of ancestors in the probands (csrc/simu.hip)
    gen.simuIdentity(ped)                  # Jacquard's nine identity coefficients of every pair by gene dropping (csrc/ident.hip)
    gen.simuRetention(ped)                 # founder allele survival, founder genome equivalents by gene dropping (csrc/retain.hip)
    gen.simuCarriers(ped, pro, controls)   # per founder allele: how many of the cases carry it, by gene dropping (csrc/carry.hip)
    gen.simuOrigins(ped, pro, groups)      # which founders the kinship and inbreeding of groups come from (csrc/origin.hip)
    gen.simuUniqueness(ped, pro, others)   # genome uniqueness of every proband: what only it carries, by gene dropping (csrc/unique.hip)
    gen.simuSharing(ped, loci=1024)        # linked loci: realised IBD sharing, its variance and the segments (csrc/link.hip)
    gen.simuSegments(ped, loci=1024)       # the lengths of those segments: histogram, within and between groups, per pair
    gen.descendant(ped, 1); gen.children(ped, 1)   # src/identify.jl:203-215, :77-80 (csrc/loader.cpp)
    gen.phiHist(ped); gen.phiQuantile(ped, 0.5)    # the distribution of the pairwise kinships, on the device (csrc/hist.hip)
    gen.phiClusters(ped, 1/16); gen.phiUnrelated(ped, 1/16)   # families and a maximal unrelated set at a kinship cutoff (csrc/clusters.hip)
    gen.phiTree(ped)                       # the single-linkage tree of the kinships: every cutoff at once (csrc/tree.hip)

All kinship arithmetic runs in hand-written HIP kernels behind the C-ABI in
include/genphi.h (csrc/genphi_hip.hip); there is no CPU fallback.
"""
import os
from collections import OrderedDict

import numpy as np

from . import _capi
from ._capi import PhiPlan, KinshipMatrix, GCPlan, OccPlan, RecPlan, DistPlan, DepthPlan, CompletenessPlan, ImplexPlan, SimuPlan, IdentityPlan, RetentionPlan, CarriersPlan, OriginsPlan, UniquenessPlan, SharingPlan, GenphiDeviceError, GenphiLibraryMissing  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)

# bundled example pedigrees (the reference exports the same names, src/GenLib.jl:27,43)
geneaJi = os.path.join(_HERE, "data", "geneaJi.csv")
genea140 = os.path.join(_HERE, "data", "genea140.csv")


class Individual:
    """What `pedigree[ID]` returns (the reference's immutable Individual, src/create.jl:39-46):
    enough of it for the path -- ID, rank, and the parents as handles (None = unknown)."""

    def __init__(self, pedigree, ID, pos):
        self.pedigree, self.ID, self.rank = pedigree, ID, pos + 1

    def _parent(self, arr):
        pid = int(arr[self.rank - 1])
        return None if pid == 0 else self.pedigree[pid]

    @property
    def father(self):
        return self._parent(self.pedigree.father)

    @property
    def mother(self):
        return self._parent(self.pedigree.mother)

    @property
    def sex(self):
        return int(self.pedigree.sex[self.rank - 1])

    def __repr__(self):
        return f"Individual({self.ID})"


class Pedigree:
    """Rank-ordered pedigree: what `gen.genealogy` returns (src/create.jl:60-74, :234-254).

    Arrays are in rank order (parents before children); `rank` of ind[k] is k + 1.
    Parent id 0 = unknown.
    """

    def __init__(self, ind, father, mother, sex):
        # (read-only, like the reference's immutable Individual structs, src/create.jl:39-46: gen.phi keeps plans per pedigree)
        self.ind, self.father, self.mother, self.sex = (np.array(a, dtype=np.int64, order="C") for a in (ind, father, mother, sex))
        for a in (self.ind, self.father, self.mother, self.sex):
            a.setflags(write=False)
        self._index = None
        self._plans = OrderedDict()          # gen.phi's plans for this pedigree, least recently used first (see _plan_for)

    def __len__(self):
        return len(self.ind)

    def __getitem__(self, ID):
        """pedigree[ID] -> Individual handle (src/create.jl:70); KeyError on an unknown ID."""
        return Individual(self, int(ID), int(self.positions([ID])[0]))

    def _idx(self):
        if self._index is None:
            order = np.argsort(self.ind, kind="stable")
            self._index = (self.ind[order], order)
        return self._index

    def positions(self, ids):
        """Rank positions of the given IDs; KeyError on an unknown ID (OrderedDict lookup)."""
        ids = np.asarray(ids, dtype=np.int64)
        keys, order = self._idx()
        k = np.searchsorted(keys, ids)
        k = np.clip(k, 0, len(keys) - 1) if len(keys) else k
        bad = (len(keys) == 0) | (keys[k] != ids) if len(ids) else np.zeros(0, bool)
        if np.any(bad):
            raise KeyError(int(ids[np.argmax(bad)]))
        return order[k]

    def __contains__(self, ID):
        keys, _ = self._idx()
        k = np.searchsorted(keys, ID)
        return k < len(keys) and keys[k] == ID

    def __repr__(self):
        return f"Pedigree({len(self)} individuals)"

    def show(self):
        """The text of the reference's Base.show(io, MIME"text/plain", pedigree) (src/create.jl:76-111), singular and plural forms
        included.  As there, whoever is not a man counts as a woman, a subject is an individual without children, and the
        generations are the depth of the deepest subject (one linear pass, csrc/loader.cpp, where the reference walks every path)."""
        n = len(self)
        relations = int(np.count_nonzero(self.father)) + int(np.count_nonzero(self.mother))
        men = int(np.count_nonzero(self.sex == 1))
        women = n - men
        subjects = len(pro(self))
        generations = _capi.genealogy_depth(self.ind, self.father, self.mother, leaves_only=True)
        s = lambda k: "" if k == 1 else "s"  # noqa: E731
        return ("A pedigree with:\n%d individual%s;\n%d parent-child relation%s;\n%d %s;\n%d %s;\n%d subject%s;\n%d generation%s."
                % (n, s(n), relations, s(relations), men, "man" if men == 1 else "men", women, "woman" if women == 1 else "women",
                   subjects, s(subjects), generations, s(generations)))


def _read_table(source):
    if isinstance(source, (str, os.PathLike)):
        # src/create.jl:161-189: header skipped, whitespace-separated ind father mother sex
        rows = np.loadtxt(source, dtype=np.int64, skiprows=1, ndmin=2)
        return rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    # DataFrame-like / mapping with the reference's column names (src/create.jl:131-146)
    get = (lambda k: np.asarray(source[k])) if not hasattr(source, "to_dict") else (lambda k: source[k].to_numpy())
    return tuple(np.asarray(get(k), dtype=np.int64) for k in ("ind", "father", "mother", "sex"))


def genealogy(source, sort=True):
    """gen.genealogy(filename | dataframe; sort=true)  (src/create.jl:131-189).

    With sort=True individuals are ordered by maximum ancestral depth (founders = 1) with a
    STABLE sort over input order (src/create.jl:196-227); the position in that order is the
    `rank` the kinship recursion branches on.  With sort=False the input order is kept and a
    parent listed after its child raises KeyError, as `_finalize_pedigree` does.
    """
    if isinstance(source, (str, os.PathLike)):
        # files go through the native loader (parse + depth sort in C++, csrc/loader.cpp)
        return Pedigree(*_capi.genealogy_read(source, sort=sort))
    # tables in memory: the same checks and the stable depth sort natively (genphi_genealogy_order, csrc/loader.cpp; the numpy form of
    # this took 1.1 s at 1e6 individuals, ten times the planning of the whole sweep)
    ind, father, mother, sex = (np.ascontiguousarray(a, dtype=np.int64) for a in _read_table(source))
    return Pedigree(*_capi.genealogy_order(ind, father, mother, sex, sort=sort))


def pro(pedigree):
    """gen.pro: IDs of individuals without children, ascending (src/identify.jl:35-39)."""
    ind, fa, mo = pedigree.ind, pedigree.father, pedigree.mother
    if len(ind) == 0:
        return ind.copy()
    lo, hi = int(ind.min()), int(ind.max())
    if lo > 0 and hi < 64 * len(ind) + (1 << 20) and int(min(fa.min(), mo.min())) >= 0 and int(max(fa.max(), mo.max())) <= hi:
        # IDs in a moderate range (genea140: 41,523 IDs up to 900,506): one flag byte per ID value instead of two sorts
        # (3-5 ms of a 12 ms gen.phi(genea140) call)
        is_parent = np.zeros(hi + 1, dtype=bool)
        is_parent[fa] = True
        is_parent[mo] = True                                 # (ID 0 = unknown parent: flagged, never looked up since lo > 0)
        return np.sort(ind[~is_parent[ind]])
    parents = np.union1d(fa, mo)
    return np.sort(ind[~np.isin(ind, parents)])


def founder(pedigree):
    """gen.founder: IDs with neither parent known, ascending (src/identify.jl:15-19)."""
    return np.sort(pedigree.ind[(pedigree.father == 0) & (pedigree.mother == 0)])


def plan(pedigree, probandIDs=None, tuning=None):
    """Levelise `pedigree` for `probandIDs` (host only; no GPU needed).  tuning: a dict of settings for this plan (PhiPlan)."""
    probandIDs = pro(pedigree) if probandIDs is None else np.asarray(probandIDs, dtype=np.int64)
    return PhiPlan(pedigree.ind, pedigree.father, pedigree.mother, probandIDs, tuning=tuning)


# gen.phi keeps the plans of its last calls per pedigree: the host prologue of the reference's phi (src/compute.jl:236-262:
# levelisation, cut sets, index copy) depends on (pedigree, probandIDs) alone, so a repeated call -- another subset, then the first one
# again; a parameter sweep -- skips planning, upload and the calibration of the sparse levels and pays the sweep and the copy.
PLAN_CACHE_ENTRIES = 4                 # per pedigree; 0 disables (also GENPHI_PLAN_CACHE=0)
PLAN_CACHE_DEVICE_BYTES = 2 << 30      # a plan that holds more device memory than this is released at the end of its call


def _plan_for(pedigree, probandIDs, device):
    """(plan, keep): the cached plan of this call, or a new one."""
    probandIDs = pro(pedigree) if probandIDs is None else np.ascontiguousarray(probandIDs, dtype=np.int64)
    entries = 0 if os.environ.get("GENPHI_PLAN_CACHE") == "0" else PLAN_CACHE_ENTRIES
    cache = getattr(pedigree, "_plans", None)
    if entries <= 0 or cache is None:
        return PhiPlan(pedigree.ind, pedigree.father, pedigree.mother, probandIDs), None
    # (the library reads its GENPHI_* hooks when a plan is created: a plan made under other settings is another plan)
    key = (hash(probandIDs.tobytes()), len(probandIDs), device, tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("GENPHI_"))))
    hit = cache.get(key)
    if hit is not None and np.array_equal(hit[1], probandIDs):
        cache.move_to_end(key)
        return hit[0], key
    return PhiPlan(pedigree.ind, pedigree.father, pedigree.mother, probandIDs), key


def _keep_plan(pedigree, key, pl, probandIDs):
    cache = pedigree._plans
    if key in cache and cache[key][0] is pl:
        return True
    if pl.device_bytes > PLAN_CACHE_DEVICE_BYTES:
        return False
    old = cache.pop(key, None)
    if old is not None:
        old[0].close()
    cache[key] = (pl, np.array(probandIDs, dtype=np.int64))
    while len(cache) > PLAN_CACHE_ENTRIES:
        cache.popitem(last=False)[1][0].close()
    return True


def phi(pedigree, probandIDs=None, verbose=False, compute=True, device=None, kernel=0):
    """gen.phi(pedigree, probandIDs = pro(pedigree); verbose=false, compute=true), or the pairwise
    method gen.phi(individual_i, individual_j) (src/compute.jl:66-95) when called with two
    `pedigree[ID]` handles: the Float64 kinship of the pair, from one Float64 level sweep on the GPU
    (the reference's recursion is un-memoised and exponential on inbred pedigrees); bit-identical to
    the recursion while kinships are exactly representable in Float64 (pedigrees less than ~26
    generations deep).  Beyond, within 2 L 2^-53 relative of the exact kinship for L level steps
    (observed: about 1 x 2^-53), and bit-identical to the same recursion memoised level by level
    wherever the result is a normal double; below 2^-1022 subnormal, within 4 x 2^-1074.

    Returns the square float32 matrix of pairwise kinship coefficients between probands
    (rows/columns in `probandIDs` order, duplicates collapsed), or None when compute=False.
    Prints the reference's cut-vertex lines (src/compute.jl:257-260, :281-284).
    Raises KeyError for an unknown proband ID.  Runs on the GPU (no CPU fallback).
    """
    if isinstance(pedigree, Individual):
        a, b = pedigree, probandIDs
        if not isinstance(b, Individual) or b.pedigree is not a.pedigree:
            raise TypeError("gen.phi(individual_i, individual_j) takes two individuals of one pedigree")
        ped = a.pedigree
        return float(_capi.phi_pairs(ped.ind, ped.father, ped.mother, [a.ID], [b.ID], device=device)[0])
    probandIDs = pro(pedigree) if probandIDs is None else np.ascontiguousarray(probandIDs, dtype=np.int64)
    pl, key = _plan_for(pedigree, probandIDs, device)
    keep = False
    try:
        if verbose or not compute:
            sizes, both = pl.levels()
            nsteps = max(len(sizes) - 1, 0)
            for i in range(nsteps):
                print(f"Step {i + 1} of {nsteps}: {sizes[i]} founders, {sizes[i + 1]} probands, {both[i]} both.")
        if not compute:
            return None
        if verbose:
            # the reference prints these inside its level loop (src/compute.jl:280-285): the library calls back right before it
            # hands each level step to the GPU
            pl.set_step_hook(lambda k, n: print(f"Running step {k + 1} of {n} ({sizes[k]} founders, {sizes[k + 1]} probands, {both[k]} both).", flush=True))
        try:
            out = pl.compute(device=device, kernel=kernel)
        finally:
            if verbose:
                pl.set_step_hook(None)               # (a hook left set would keep the plan off its captured graph)
        keep = key is not None and _keep_plan(pedigree, key, pl, probandIDs)
        return out
    finally:
        if not keep:
            if key is not None and key in pedigree._plans and pedigree._plans[key][0] is pl:
                del pedigree._plans[key]             # (a cached plan whose call failed)
            pl.close()


def f(pedigree, IDs, device=None):
    """gen.f(pedigree, IDs) (src/compute.jl:500-511): inbreeding coefficients (Float32 vector).

    F(x) = kinship of x's parents, 0 if a parent is unknown.  The reference evaluates each one
    with the un-memoised Float64 pairwise recursion (:66-95), exponential on deep inbred
    pedigrees, and rounds the result to Float32 once.  Here ONE level sweep over the set of
    parents runs on the GPU with Float64 level matrices (GENPHI_FLAG_STORAGE_F64), the
    (father, mother) entries are read back (`genphi_result_entries`) and rounded to Float32 once:
    the same values bit for bit while kinships are exactly representable in Float64 (pedigrees
    less than ~26 generations deep; beyond, within 2 L 2^-53 relative of the exact kinship before
    the rounding, L = level steps: within 1 Float32 ulp of the correctly rounded value after it).
    test/runtests.jl:47-48: f(ped, [1]) == [0.18359375], f(ped, [17]) == [0.].
    """
    IDs = np.asarray(IDs, dtype=np.int64)
    pos = pedigree.positions(IDs)                       # KeyError on an unknown ID
    fa, mo = pedigree.father[pos], pedigree.mother[pos]
    out = np.zeros(len(IDs), dtype=np.float32)
    both = (fa != 0) & (mo != 0)
    if not np.any(both):
        return out
    parents = np.unique(np.concatenate([fa[both], mo[both]]))     # sorted, like a proband list
    pl, key = _plan_for(pedigree, parents, device)                # (kept per pedigree like gen.phi's plans: f over the same IDs again pays the sweep)
    keep = False
    try:
        pl.compute_device(device=device, storage64=True)
        out[both] = pl.result_entries(np.searchsorted(parents, fa[both]), np.searchsorted(parents, mo[both])).astype(np.float32)
        keep = key is not None and _keep_plan(pedigree, key, pl, parents)
    finally:
        if not keep:
            if key is not None and key in pedigree._plans and pedigree._plans[key][0] is pl:
                del pedigree._plans[key]
            pl.close()
    return out


def branching(pedigree, pro=None, ancestors=None):
    """gen.branching(pedigree; pro=nothing, ancestors=nothing) (src/extract.jl:65-186).

    Pedigree of the individuals on the paths between the selected probands and ancestors
    (host-side pruning before gen.phi; native, csrc/loader.cpp).  KeyError on an unknown ID.
    """
    return Pedigree(*_capi.branching(pedigree.ind, pedigree.father, pedigree.mother, pedigree.sex,
                                     pro=pro, ancestors=ancestors))


def gc(pedigree, pro=None, ancestors=None, device=None):
    """gen.gc(pedigree; pro = pro(pedigree), ancestors = founder(pedigree)) (src/compute.jl:518-595): the genetic
    contribution of each ancestor (columns) to each proband (rows), a float32 array of shape (len(pro), len(ancestors)).

    Entry [i, j] = sum over the descending paths from ancestors[j] to pro[i] of 0.5^length, computed on the GPU by a
    Float64 recursion over the generation cuts (csrc/gc.hip) and rounded to float32 once.  As in the reference, only
    leaves (individuals without children) receive contributions, and a proband listed again gets a row of zeros.  Equal
    to the reference bit for bit while the sweep has at most 24 steps; deeper, the correctly rounded exact value (up to
    52 steps; within 1 ulp beyond), where the reference's own path-by-path float32 sums may round differently
    (include/genphi.h).  KeyError for an unknown ID.  Each call plans, sweeps and frees its own handle."""
    probands = globals()["pro"](pedigree) if pro is None else np.ascontiguousarray(pro, dtype=np.int64)
    ancestors = founder(pedigree) if ancestors is None else np.ascontiguousarray(ancestors, dtype=np.int64)
    h = GCPlan(pedigree.ind, pedigree.father, pedigree.mother, probands, ancestors)
    try:
        h.compute(device=device)
        return h.result_to_host()
    finally:
        h.close()


def occ(pedigree, pro=None, ancestors=None, typeOcc="IND", device=None):
    """gen.occ(pedigree; pro = pro(pedigree), ancestors = founder(pedigree), typeOcc = "IND") (src/describe.jl:184-238): how
    many times each ancestor (rows) occurs in each proband's genealogy (columns), an int64 array of shape
    (len(ancestors), len(pro)); typeOcc = "TOTAL": summed over the probands, shape (len(ancestors), 1).

    Entry [j, i] = the number of ascending paths from pro[i] to ancestors[j] (1 for the proband itself), computed on the GPU
    by an integer recursion over the generation cuts (csrc/occ.hip) with the reference's wrap-around: equal to the
    reference bit for bit at any depth.  The "IND" array is a transposed view of the (len(pro), len(ancestors)) row-major
    result, not a copy.  "TOTAL" is reduced on the device and never holds the full matrix.  As in the reference, every
    proband counts (with or without children, each time it is listed), and of a duplicated ancestor only the first row
    carries values.  KeyError for an unknown ID; ValueError for another typeOcc (the reference returns nothing).  Each call
    plans, sweeps and frees its own handle."""
    if typeOcc not in ("IND", "TOTAL"):
        raise ValueError('typeOcc must be "IND" or "TOTAL", not %r' % (typeOcc,))
    probands = globals()["pro"](pedigree) if pro is None else np.ascontiguousarray(pro, dtype=np.int64)
    ancestors = founder(pedigree) if ancestors is None else np.ascontiguousarray(ancestors, dtype=np.int64)
    h = OccPlan(pedigree.ind, pedigree.father, pedigree.mother, probands, ancestors, total_only=typeOcc == "TOTAL")
    try:
        h.compute(device=device)
        return h.totals().reshape(-1, 1) if typeOcc == "TOTAL" else h.result_to_host().T
    finally:
        h.close()


def rec(pedigree, probandIDs=None, ancestorIDs=None, device=None):
    """gen.rec(pedigree, probandIDs = pro(pedigree), ancestorIDs = founder(pedigree)) (src/describe.jl:133-145): the coverage
    of each ancestor, that is, how many of the probands descend from it; an int64 array of length len(ancestorIDs).

    Computed on the GPU as ancestor bit sets by an OR recursion over the generation cuts and a column count over the
    probands' rows (csrc/occ.hip); not derived from gen.occ, whose counts can wrap to 0.  As in the reference, descendants
    are strict (an ancestor that is a proband does not count itself), a proband listed twice counts once, a proband ID that
    is not in the pedigree is ignored, and a duplicated ancestor gives equal entries.  KeyError for an unknown ancestor ID."""
    probandIDs = pro(pedigree) if probandIDs is None else np.ascontiguousarray(probandIDs, dtype=np.int64)
    ancestorIDs = founder(pedigree) if ancestorIDs is None else np.ascontiguousarray(ancestorIDs, dtype=np.int64)
    h = RecPlan(pedigree.ind, pedigree.father, pedigree.mother, probandIDs, ancestorIDs)
    try:
        h.compute(device=device)
        return h.result()
    finally:
        h.close()


def meioses(pedigree, pro=None, ancestors=None, device=None):
    """gen.meioses(pedigree; pro = pro(pedigree), ancestors = founder(pedigree)): the number of meioses on the shortest ascending
    path from each proband (rows) to each ancestor (columns), an int16 array of shape (len(pro), len(ancestors)); 0 where the
    proband is the ancestor, -1 where the ancestor is not an ancestor of the proband.

    The reference has no matrix form of this: it is _findMinDistance (src/describe.jl:283-289) for every pair at once, computed on
    the GPU by a min-plus recursion over the generation cuts (csrc/dist.hip) instead of an enumeration of every path.  Every
    proband gets its row (with or without children, each time it is listed); a duplicated ancestor gives equal columns.  KeyError
    for an unknown ID; ValueError for a pedigree of more than 32,767 generation steps.  Each call plans, sweeps and frees its own
    handle."""
    probands = globals()["pro"](pedigree) if pro is None else np.ascontiguousarray(pro, dtype=np.int64)
    ancestors = founder(pedigree) if ancestors is None else np.ascontiguousarray(ancestors, dtype=np.int64)
    h = DistPlan(pedigree.ind, pedigree.father, pedigree.mother, probands, ancestors)
    try:
        h.compute(device=device)
        return h.result_to_host()
    finally:
        h.close()


class GenDepths:
    """What gen.depths returns: `pro` and `ancestors` as given, `by`, and the arrays `min`, `max` (int16, -1 = no path), `mean`
    (float64, NaN = no path) and `paths` (int64), of shape (len(pro), len(ancestors)) for by="pair", (len(pro),) for by="proband"
    and (len(ancestors),) for by="ancestor"."""

    def __init__(self, pro, ancestors, by, min, max, mean, paths):
        self.pro, self.ancestors, self.by = pro, ancestors, by
        self.min, self.max, self.mean, self.paths = min, max, mean, paths

    def __repr__(self):
        return "GenDepths(by=%r, %d probands, %d ancestors)" % (self.by, len(self.pro), len(self.ancestors))


def depths(pedigree, pro=None, ancestors=None, by="pair", device=None):
    """gen.depths(pedigree; pro = pro(pedigree), ancestors = founder(pedigree), by = "pair"): over ALL ascending paths from each
    proband (rows) to each ancestor (columns), their number (`paths`), the meioses of the shortest and of the longest (`min`, `max`)
    and the mean number of meioses (`mean`), as a GenDepths.  The empty path counts where the proband is the ancestor (1, 0, 0, 0.0);
    where the ancestor is not an ancestor of the proband: paths 0, min = max = -1, mean NaN.

    This is the reference's _findDistance (src/describe.jl:241-279), which returns the length of every ascending path between a
    descendant and an ancestor, reduced to its count, minimum, maximum and mean -- for every pair at once, by one exact integer
    recursion over the generation cuts on the GPU (csrc/depth.hip) instead of an enumeration of every path.  `min` equals
    gen.meioses, `paths` equals gen.occ(...).T without its wrap-around, and mean is the correctly rounded quotient of the exact sum
    of the lengths and the exact count.  by="proband" reduces over the ancestors on the device (all paths from the proband to any
    listed ancestor: vectors of len(pro)), by="ancestor" over the probands (vectors of len(ancestors); no pair matrix exists);
    both combine integers only, and their mean is float(sum of lengths) / float(paths).

    Every listed proband gets its row (with or without children, each time it is listed); under by="pair" and by="ancestor" a
    duplicated ancestor gives equal entries.  KeyError for an unknown ID.  ValueError for a pedigree of more than 47 generation
    steps above the probands (the packed count holds 2^47 paths per pair), for a duplicated ancestor under by="proband" (a path
    would be added twice), for by="ancestor" where len(pro) * steps * 2^steps reaches 2^63 (the sums could exceed Int64), and for
    another `by`.  Each call plans, sweeps and frees its own handle."""
    probands = globals()["pro"](pedigree) if pro is None else np.ascontiguousarray(pro, dtype=np.int64)
    ancestors = founder(pedigree) if ancestors is None else np.ascontiguousarray(ancestors, dtype=np.int64)
    h = DepthPlan(pedigree.ind, pedigree.father, pedigree.mother, probands, ancestors, by=by)
    try:
        h.compute(device=device)
        lo, hi, paths, mean = h.result_to_host()
        return GenDepths(probands, ancestors, by, lo, hi, mean, paths)
    finally:
        h.close()


def _founder_depths(pedigree, individuals, device):
    individuals = globals()["pro"](pedigree) if individuals is None else _id_list(individuals)
    return depths(pedigree, individuals, founder(pedigree), by="proband", device=device)


def genMin(pedigree, individuals=None, device=None):
    """GENLIB's gen.min(gen, individuals): for each individual the generations to its NEAREST founder, the shortest of all its
    ascending paths to any founder (0 for a founder); int16.  gen.depths(..., by="proband").min over all founders.  Not named `min`:
    a module-level name would shadow the builtin this module itself uses.  The orientation (one entry per listed individual) and
    the definition are this package's own."""
    return _founder_depths(pedigree, individuals, device).min


def genMax(pedigree, individuals=None, device=None):
    """GENLIB's gen.max(gen, individuals): for each individual the generations to its FARTHEST founder, the longest of all its
    ascending paths to any founder (0 for a founder); int16.  gen.depths(..., by="proband").max over all founders.  Not named `max`:
    a module-level name would shadow the builtin this module itself uses.  The orientation and the definition are this package's
    own."""
    return _founder_depths(pedigree, individuals, device).max


def genMean(pedigree, individuals=None, device=None):
    """GENLIB's gen.mean(gen, individuals): for each individual the mean number of generations over ALL its ascending paths to
    founders (0.0 for a founder), every path with weight one; float64, float(sum of the lengths) / float(number of paths).
    gen.depths(..., by="proband").mean over all founders.  Not named `mean`, like gen.genMin and gen.genMax beside it (`min` and
    `max` would shadow builtins the module itself uses).  The orientation and the definition are this package's own."""
    return _founder_depths(pedigree, individuals, device).mean


def completeness(pedigree, pro=None, genNo=None, type="MEAN", device=None):
    """gen.completeness(pedigree, pro = pro(pedigree); genNo = Int[], type = "MEAN") (src/describe.jl:73-125): the completeness of
    the probands' genealogies per generation (rows; the probands are generation 0), in percent: the known ancestors of
    generation g, counted with multiplicity, out of 2^g.  type = "IND": a float64 array of shape (G, len(pro)), one column per
    proband, G = 1 + the longest ascent of any listed proband; type = "MEAN" (the default): the mean over the probands, (G, 1).
    genNo: the generations to return, in the order given, repeats allowed.

    The counts are the number of ascending paths of exactly g meioses, computed on the GPU by an Int64 recursion over the
    generation cuts (csrc/completeness.hip) where the reference walks every path; "IND" is converted on the device by the
    reference's own operations (count / 2^g * 100) and is equal to the reference bit for bit.  It is a transposed view of the
    (len(pro), G) row-major result, not a copy.  "MEAN" is formed from the per-generation totals, reduced on the device:
    mean[g] = float(totals[g]) / 2^g * 100 / len(pro).  Every entry of the reference's matrix is 25 count / 2^(g - 2), exact in
    Float64 while 25 count < 2^53, and so is every partial sum of a row while 25 totals[g] < 2^53: the reference's sequential
    sum is then exact and the only rounding is the final division.  So "MEAN" is bit-identical to the reference whenever
    25 totals[g] < 2^53 for every g (for example 1e5 probands down to 30 generations); beyond that it is within 2 ulp of the exact
    rational mean (three roundings of half an ulp), where the reference's own sequential sum can be off by up to len(pro) / 2
    ulp.  Where the totals could exceed Int64 ((G - 1) + ceil(log2(len(pro))) > 62), "MEAN" is the sequential sum of the "IND"
    result in proband order, as in the reference.

    As in the reference every proband gets its column (with or without children, each time it is listed).  KeyError for an
    unknown proband; ValueError for an empty pro (the reference's maximum of an empty collection throws), for another type (the
    reference returns nothing) and for more than 62 generations above the probands (the reference's 2^g overflows there);
    IndexError for a generation outside 0 .. G - 1 (the reference's BoundsError).  Each call plans, sweeps and frees its own
    handle."""
    if type not in ("IND", "MEAN"):
        raise ValueError('type must be "IND" or "MEAN", not %r' % (type,))
    probands = globals()["pro"](pedigree) if pro is None else np.ascontiguousarray(pro, dtype=np.int64)
    if len(probands) == 0:
        raise ValueError("gen.completeness needs at least one proband")
    args = (pedigree.ind, pedigree.father, pedigree.mother, probands)
    h = None
    if type == "MEAN":
        try:
            h = CompletenessPlan(*args, totals_only=True)
        except ValueError:
            h = None                                      # too deep (raised again below), or the totals could exceed Int64
    if h is None:
        h = CompletenessPlan(*args)
    try:
        G = h.generations
        rows = None
        if genNo is not None and len(genNo):
            rows = np.asarray(genNo, dtype=np.int64).ravel()
            if np.any((rows < 0) | (rows >= G)):
                raise IndexError("generation %d is outside 0 .. %d" % (int(rows[(rows < 0) | (rows >= G)][0]), G - 1))
        h.compute(device=device)
        if type == "IND":
            out = h.result_to_host().T
        elif h.totals_only:
            out = (h.totals().astype(np.float64) / np.ldexp(1.0, np.arange(G)) * 100.0 / len(probands)).reshape(-1, 1)
        else:
            out = (np.cumsum(h.result_to_host(), axis=0)[-1] / len(probands)).reshape(-1, 1)     # a sequential sum, proband order
        return out if rows is None else out[rows, :]
    finally:
        h.close()


def implex(pedigree, pro=None, genNo=None, type="MEAN", onlyNewAnc=False, device=None):
    """gen.implex(pedigree, pro = pro(pedigree); genNo = Int[], type = "MEAN", onlyNewAnc = false), GENLIB's gen.implex (the
    reference has no form of it): the genealogical implex of the probands per generation (rows; the probands are generation 0), in
    percent: the DISTINCT ancestors of generation g out of 2^g, where gen.completeness counts them with multiplicity; the gap
    between the two curves is the pedigree collapse.  With A_0(p) = {p} and A_{g+1}(p) = the known parents of the members of
    A_g(p), the count is |A_g(p)| (an individual can be in several A_g(p): generations overlap); onlyNewAnc=True counts
    |A_g \\ (A_0 u .. u A_{g-1})|, every individual in the generation of its shortest ascent only.  type = "IND": a float64 array of
    shape (G, len(pro)), one column per proband, G = 1 + the longest ascent of any listed proband (as gen.completeness);
    type = "MEAN" (the default): the mean over the probands, (G, 1).  genNo: the generations to return, in the order given,
    repeats allowed.

    The counts come from a level-synchronous frontier over bit rows on the GPU (csrc/implex.hip): rows are individuals, columns
    the listed probands as bits, and generation g ORs the rows of an individual's children of generation g - 1.  "IND" is
    converted on the device by count / 2^g * 100 in that order and is a transposed view of the (len(pro), G) row-major result,
    not a copy.  "MEAN" is float(totals[g]) / 2^g * 100 / len(pro) from the totals reduced on the device; totals[g] <=
    len(pro) x the number of individuals, so 25 totals[g] < 2^53, everything before the division is exact and "MEAN" is the
    correctly rounded exact rational mean.

    Every proband gets its column (with or without children, each time it is listed).  KeyError for an unknown proband; ValueError
    for an empty pro, for another type (GENLIB's "ALL" included) and for more than 62 generations above the probands; IndexError
    for a generation outside 0 .. G - 1.  Each call plans, sweeps and frees its own handle."""
    if type not in ("IND", "MEAN"):
        raise ValueError('type must be "IND" or "MEAN", not %r' % (type,))
    probands = globals()["pro"](pedigree) if pro is None else np.ascontiguousarray(pro, dtype=np.int64)
    if len(probands) == 0:
        raise ValueError("gen.implex needs at least one proband")
    h = ImplexPlan(pedigree.ind, pedigree.father, pedigree.mother, probands, only_new=bool(onlyNewAnc))
    try:
        G = h.generations
        rows = None
        if genNo is not None and len(genNo):
            rows = np.asarray(genNo, dtype=np.int64).ravel()
            if np.any((rows < 0) | (rows >= G)):
                raise IndexError("generation %d is outside 0 .. %d" % (int(rows[(rows < 0) | (rows >= G)][0]), G - 1))
        h.compute(device=device)
        if type == "IND":
            out = h.result_to_host().T
        else:
            out = (h.totals().astype(np.float64) / np.ldexp(1.0, np.arange(G)) * 100.0 / len(probands)).reshape(-1, 1)
        return out if rows is None else out[rows, :]
    finally:
        h.close()


def _simu_plan(pedigree, pro, ancestors, stateAncestors, simulNo, seed, no_sample):
    probands = globals()["pro"](pedigree) if pro is None else np.ascontiguousarray(pro, dtype=np.int64)
    ancestors = founder(pedigree) if ancestors is None else np.ascontiguousarray(ancestors, dtype=np.int64)
    states = np.ones(len(ancestors), dtype=np.int32) if stateAncestors is None else stateAncestors
    return SimuPlan(pedigree.ind, pedigree.father, pedigree.mother, probands, ancestors, states, simul_no=simulNo, seed=seed,
                    no_sample=no_sample)


def simuSample(pedigree, pro=None, ancestors=None, stateAncestors=None, simulNo=5000, seed=None, device=None):
    """gen.simuSample(pedigree, pro = pro(pedigree), ancestors = founder(pedigree), stateAncestors = all 1, simulNo = 5000), GENLIB's
    gen.simuSample (the reference has no form of it): gene dropping.  Every ancestor carries stateAncestors[j] in {0, 1, 2} copies
    of a marked allele; the alleles are dropped down the pedigree simulNo times, every meiosis passing on the paternal or the
    maternal copy with probability 1/2.  Returns the int8 array of shape (len(pro), simulNo): the copies proband i carries in
    simulation s.

    A listed ancestor keeps its state in every simulation and blocks every path through it (its own parents are ignored, a
    state-0 ancestor included).  The random bits are Philox4x32-10 keyed on (seed, the individual's ID, the parental side, the
    absolute word of 64 simulations): the result is a pure function of the pedigree's relations, the ancestors with their states
    and the seed (include/genphi.h) -- simulNo = 64 gives the first 64 columns of simulNo = 5000, a sub-list of probands gives
    the same rows, and gen.branching(pedigree, pro=.., ancestors=..) first changes no row of the probands it keeps.  (Pruning drops
    a proband that descends from no listed ancestor, whose row is zero, and an ancestor above no listed proband, which marks
    no row; passing a dropped ID with the pruned pedigree is a KeyError, so pass the kept ones.)  seed=None draws 64 fresh bits (secrets.randbits); pass a seed to
    repeat a run.  The sweep runs on the GPU, 64 simulations per word, level by level from the ancestors down (csrc/simu.hip).

    GENLIB's probRecomb and probSurvival are not offered.  KeyError for an unknown ID; ValueError for a state outside 0..2, lists of
    different length, an ancestor listed with two states, simulNo outside 1 .. 2^24, an empty pro or no ancestors.  Each call
    plans, sweeps and frees its own handle."""
    h = _simu_plan(pedigree, pro, ancestors, stateAncestors, simulNo, seed, False)
    try:
        h.compute(device=device)
        return h.sample_to_host()
    finally:
        h.close()


class SimuProb:
    """What gen.simuProb returns: joint, the share of the simulations in which every proband i carries statePro[i] copies;
    marginal[i], the share in which proband i does; by_number[k], the share in which exactly k probands do; simulNo and the seed
    used.  Every probability is an integer count divided by simulNo once."""

    def __init__(self, joint, marginal, by_number, simulNo, seed):
        self.joint, self.marginal, self.by_number, self.simulNo, self.seed = joint, marginal, by_number, simulNo, seed

    def __repr__(self):
        return "SimuProb(joint=%r, simulNo=%d, seed=%d)" % (self.joint, self.simulNo, self.seed)


def simuProb(pedigree, pro, statePro, ancestors, stateAncestors, simulNo=5000, seed=None, device=None):
    """gen.simuProb(pedigree, pro, statePro, ancestors, stateAncestors, simulNo = 5000), GENLIB's gen.simuProb (the reference has no
    form of it): the probability, estimated by gene dropping (gen.simuSample, with its rules, seed and errors), that proband i
    carries statePro[i] in {0, 1, 2} copies of the alleles that the ancestors carry.  Returns a SimuProb: joint (all probands at
    once), marginal (each proband alone) and by_number (exactly k of them, k = 0 .. len(pro)).

    Counted on the GPU from the bit rows of the sweep (csrc/simu.hip); no (len(pro), simulNo) sample is ever held.  Each call
    plans, sweeps and frees its own handle."""
    h = _simu_plan(pedigree, pro, ancestors, stateAncestors, simulNo, seed, True)
    try:
        statePro = np.asarray(statePro).ravel()
        if len(statePro) != h.n_pro:
            raise ValueError("gen.simuProb: %d probands but %d states" % (h.n_pro, len(statePro)))
        if len(statePro) and (not np.array_equal(statePro, statePro.astype(np.int64)) or statePro.min() < 0 or statePro.max() > 2):
            raise ValueError("gen.simuProb: statePro must be 0, 1 or 2")
        statePro = statePro.astype(np.int64)
        h.compute(device=device)
        S = h.simul_no
        marginal = h.state_counts()[np.arange(h.n_pro), statePro] / float(S)
        by_number = np.bincount(h.match_counts(statePro), minlength=h.n_pro + 1) / float(S)
        return SimuProb(float(by_number[-1]), marginal, by_number, S, h.seed)
    finally:
        h.close()


class SimuIdentity:
    """What gen.simuIdentity returns.  pro: the listed probands; counts: int32 (N, N, 9), the simulations in which the ordered
    pair (i, j) is in Jacquard's condensed state k + 1; simulNo and the seed used; alleles: int64 (n_labels, 2), the ID and the
    side (0 = from the father) of every founder allele, in label order; labels: int32 (N, 2, simulNo), the labels of the two
    sides of every proband, or None.  Every coefficient below is an integer count divided by simulNo once, in Float64."""

    def __init__(self, pro, counts, simulNo, seed, alleles, labels):
        self.pro, self.counts, self.simulNo, self.seed, self.alleles, self.labels = pro, counts, simulNo, seed, alleles, labels

    def __repr__(self):
        return "SimuIdentity(%d probands, simulNo=%d, seed=%d)" % (len(self.pro), self.simulNo, self.seed)

    @property
    def delta(self):
        """(N, N, 9): the estimates of the identity coefficients D1 .. D9."""
        return self.counts / float(self.simulNo)

    @property
    def kinship(self):
        """(N, N): D1 + (D3 + D5 + D7) / 2 + D8 / 4."""
        c = self.counts.astype(np.int64)
        return (4 * c[..., 0] + 2 * (c[..., 2] + c[..., 4] + c[..., 6]) + c[..., 7]) / (4.0 * self.simulNo)

    @property
    def inbreeding(self):
        """(N,): the share of the simulations in which the two alleles of proband i are identical by descent."""
        n = np.arange(len(self.pro))
        return self.counts[n, n, 0] / float(self.simulNo)

    @property
    def fraternity(self):
        """(N, N): D7, the dominance relationship; valid under inbreeding."""
        return self.counts[..., 6] / float(self.simulNo)

    @property
    def ibd(self):
        """(N, N, 3): the shares of the simulations with 0, 1, 2 alleles shared in the non-inbred states 9, 8, 7."""
        return self.counts[..., [8, 7, 6]] / float(self.simulNo)

    @property
    def inbred(self):
        """(N, N): D1 + .. + D6, the share of the simulations in which either of the two is inbred: what ibd leaves out."""
        return self.counts[..., :6].sum(axis=-1, dtype=np.int64) / float(self.simulNo)


def simuIdentity(pedigree, pro=None, simulNo=5000, seed=None, labels=False, device=None):
    """gen.simuIdentity(pedigree, pro = pro(pedigree), simulNo = 5000): Jacquard's nine condensed identity coefficients of every
    ordered pair of probands (Chapman & Jacquard 1971 studied them on the bundled geneaJi), estimated by gene dropping: every
    founder allele is dropped down the pedigree under its own label simulNo times, and the identity state of every pair is read
    off in every simulation.  Returns a SimuIdentity: counts, and from them delta, kinship, inbreeding, fraternity, ibd, inbred.

    The random bits are those of gen.simuSample (Philox4x32-10 keyed on the seed, the individual's ID, the parental side and the
    absolute word of 64 simulations): the result is a pure function of the pedigree's relations, the probands, the seed and
    simulNo (include/genphi.h); a sub-list of probands gives the sub-block and gen.branching(pedigree, pro=..) first changes
    nothing.  seed=None draws 64 fresh bits; pass a seed to repeat a run.  labels=True also returns the probands' labels.  The
    sweep and the pair counts run on the GPU (csrc/ident.hip).

    KeyError for an unknown ID; ValueError for simulNo outside 1 .. 2^24, an empty pro, or 2^31 or more ordered pairs.  Each call
    plans, sweeps and frees its own handle."""
    probands = globals()["pro"](pedigree) if pro is None else np.ascontiguousarray(pro, dtype=np.int64)
    h = IdentityPlan(pedigree.ind, pedigree.father, pedigree.mother, probands, simul_no=simulNo, seed=seed, labels=labels)
    try:
        h.compute(device=device)
        return SimuIdentity(probands, h.counts_to_host(), h.simul_no, h.seed, h.alleles(), h.labels_to_host() if labels else None)
    finally:
        h.close()


class SimuRetention:
    """What gen.simuRetention returns.  pro: the listed probands; alleles: int64 (n_labels, 2), the ID and the side (0 = from the
    father) of every founder allele, in label order; survived, both: int32 (n_labels,); distinct: int32 (simulNo,) (the definition is
    the text of genphi_retain_* in include/genphi.h); simulNo and the seed used.  Every share below is formed once from the integers,
    in Float64.  p: the expected frequency of every founder allele among the proband genes, or None (contributions=False)."""

    def __init__(self, pro, alleles, survived, both, distinct, simulNo, seed, p=None):
        self.pro, self.alleles, self.survived, self.both, self.distinct = pro, alleles, survived, both, distinct
        self.simulNo, self.seed, self.p = simulNo, seed, p
        ids = alleles[:, 0]
        first = np.ones(len(ids), dtype=bool)
        first[1:] = ids[1:] != ids[:-1]
        self._first = np.flatnonzero(first)                        # the label of every founder's first allele
        self._two = np.diff(np.append(self._first, len(ids))) == 2

    def __repr__(self):
        return "SimuRetention(%d probands, %d founder alleles, simulNo=%d, seed=%d)" % (len(self.pro), len(self.alleles), self.simulNo, self.seed)

    @property
    def retention(self):
        """(n_labels,): the share of the simulations in which the allele survives in at least one proband."""
        return self.survived / float(self.simulNo)

    @property
    def founders(self):
        """The IDs of the allele table, ascending: the founders and half-founders of the live set."""
        return self.alleles[self._first, 0]

    @property
    def n_alleles(self):
        """Per founder: 2, or 1 for a half-founder."""
        return np.where(self._two, 2, 1)

    def _sums(self):
        s = self.survived.astype(np.int64)
        second = np.where(self._two, s[np.minimum(self._first + 1, len(s) - 1)], 0)
        return s[self._first], second, np.where(self._two, self.both[self._first].astype(np.int64), 0)

    @property
    def kept(self):
        """Per founder: the mean retention of its alleles."""
        a, b, _ = self._sums()
        return (a + b) / (self.n_alleles * float(self.simulNo))

    @property
    def lost(self):
        """Per founder: the share of the simulations in which none of its alleles survives."""
        a, b, ab = self._sums()
        return (self.simulNo - (a + b - ab)) / float(self.simulNo)

    @property
    def whole(self):
        """Per founder: the share of the simulations in which both of its alleles survive; NaN for a half-founder."""
        ab = self._sums()[2]
        return np.where(self._two, ab / float(self.simulNo), np.nan)

    @property
    def alleles_mean(self):
        """The mean number of distinct founder alleles left in a simulation."""
        return int(self.survived.sum(dtype=np.int64)) / float(self.simulNo)

    @property
    def alleles_sd(self):
        """The standard deviation (over the simulations, divisor simulNo) of the number of distinct founder alleles left."""
        d = self.distinct.astype(np.int64)
        n = self.simulNo
        return float(np.sqrt(max(n * int((d * d).sum()) - int(d.sum()) ** 2, 0)) / n)

    @property
    def hist(self):
        """hist[k]: the simulations with exactly k distinct founder alleles left."""
        return np.bincount(self.distinct)

    @property
    def fe(self):
        """The founder equivalents 1 / (2 sum p^2) (Lacy 1989); None without contributions."""
        return None if self.p is None else 1.0 / (2.0 * float(np.sum(self.p * self.p)))

    @property
    def fg_dropped(self):
        """The alleles with retention 0 that the fg sum leaves out."""
        return int(np.count_nonzero(self.survived == 0))

    @property
    def fg(self):
        """Lacy's founder genome equivalents 1 / (2 sum p^2 / retention) over the alleles with retention > 0; None without
        contributions."""
        if self.p is None:
            return None
        k = self.survived > 0
        return 1.0 / (2.0 * float(np.sum(self.p[k] * self.p[k] * (float(self.simulNo) / self.survived[k]))))


def simuRetention(pedigree, pro=None, simulNo=5000, seed=None, contributions=True, device=None):
    """gen.simuRetention(pedigree, pro = pro(pedigree), simulNo = 5000): which founder alleles are still present in the probands,
    and how many (MacCluer et al. 1986), estimated by gene dropping: every founder allele is dropped down the pedigree under its own
    label simulNo times (the labels of gen.simuIdentity under the same seed), and in every simulation the labels the probands carry
    are marked.  Returns a SimuRetention: per founder allele survived and retention; per founder kept, lost and whole; per
    simulation distinct, with alleles_mean, alleles_sd and hist; and, with contributions=True, p, the exact expected frequency of
    every founder allele among the 2 n genes of the n different listed probands (sum_i gen.gc(i, founder) / (2 n), with gen.gc's
    rule that only individuals without children receive contributions; it sums to 1 for such probands), the founder equivalents fe
    and Lacy's founder genome equivalents fg.

    The result is a pure function of the pedigree's relations, the set of listed probands (order and repeats change nothing), the
    seed and simulNo (include/genphi.h); gen.branching(pedigree, pro=..) first changes nothing.  seed=None draws 64 fresh bits; pass
    a seed to repeat a run.  The sweep and the reduction run on the GPU (csrc/retain.hip); only 2 n_labels + simulNo integers come
    back, and any number of probands is taken.

    KeyError for an unknown ID; ValueError for simulNo outside 1 .. 2^24 or an empty pro.  Each call plans, sweeps and frees its
    own handles."""
    probands = globals()["pro"](pedigree) if pro is None else np.ascontiguousarray(pro, dtype=np.int64)
    h = RetentionPlan(pedigree.ind, pedigree.father, pedigree.mother, probands, simul_no=simulNo, seed=seed)
    try:
        h.compute(device=device)
        alleles = h.alleles()
        p = None
        if contributions:
            listed = np.unique(probands)
            ids, inverse = np.unique(alleles[:, 0], return_inverse=True)
            c = gc(pedigree, pro=listed, ancestors=ids, device=device).astype(np.float64).sum(axis=0)
            p = c[inverse] / (2.0 * len(listed))
        return SimuRetention(probands, alleles, h.survived_to_host(), h.both_to_host(), h.distinct_to_host(), h.simul_no, h.seed, p)
    finally:
        h.close()


class SimuCarriers:
    """What gen.simuCarriers returns.  pro: the distinct cases, ascending; controls: the distinct controls, ascending; alleles: int64
    (n_labels, 2), the ID and the side (0 = from the father) of every founder allele, in label order; carriers, homozygotes: int32
    (n_labels, W); excluded: int32 (n_labels,) (the definition is the text of genphi_carry_* in include/genphi.h; column 0 of both
    tables is filled here: the simulations in which no control and no case carries the allele); simulNo and the seed used.  With
    n = len(pro), W = n + 1 unless maxCount < n cut the tables: then the last column lumps every count >= maxCount, and what needs the
    exact count n is None.  Every share below is formed once from the integers, in Float64."""

    def __init__(self, pro, controls, alleles, carriers, homozygotes, excluded, simulNo, seed):
        self.pro, self.controls, self.alleles = pro, controls, alleles
        self.carriers, self.homozygotes, self.excluded = carriers, homozygotes, excluded
        self.simulNo, self.seed = simulNo, seed
        self.lumped = carriers.shape[1] - 1 < len(pro)

    def __repr__(self):
        return "SimuCarriers(%d cases, %d controls, %d founder alleles, simulNo=%d, seed=%d)" % (len(self.pro), len(self.controls), len(self.alleles),
                                                                                                self.simulNo, self.seed)

    @property
    def founders(self):
        """The IDs of the allele table, ascending: the founders and half-founders of the live set."""
        return np.unique(self.alleles[:, 0])

    def at_least(self, k, homozygous=False):
        """(n_labels,): the share of the simulations in which no control and at least k cases carry the allele (homozygous: on both
        sides).  ValueError for k < 0, or for k beyond the last column of lumped tables."""
        table = self.homozygotes if homozygous else self.carriers
        k = int(k)
        if k < 0 or (self.lumped and k >= table.shape[1]):
            raise ValueError("gen.simuCarriers: at_least(%d) with columns 0 .. %d%s" % (k, table.shape[1] - 1, " (the last one lumped)" if self.lumped else ""))
        return table[:, k:].sum(axis=1, dtype=np.int64) / float(self.simulNo)

    @property
    def mean_carriers(self):
        """(n_labels,): the mean number of cases that carry the allele, simulations with a carrying control counted as 0; None when
        the last column lumps."""
        if self.lumped:
            return None
        return (self.carriers.astype(np.int64) @ np.arange(self.carriers.shape[1], dtype=np.int64)) / float(self.simulNo)

    @property
    def prob_all(self):
        """(n_labels,): the share of the simulations in which every case and no control carries the allele; None when the last
        column lumps."""
        return None if self.lumped else self.carriers[:, -1] / float(self.simulNo)

    @property
    def prob_all_hom(self):
        """(n_labels,): the same with every case carrying it on both sides."""
        return None if self.lumped else self.homozygotes[:, -1] / float(self.simulNo)

    @property
    def posterior(self):
        """(n_labels,): prob_all / prob_all.sum(), the posterior of which founder allele introduced a variant that every case and
        no control carries, under a uniform prior over the founder alleles; zeros when no simulation had such an allele."""
        if self.lumped:
            return None
        last = self.carriers[:, -1].astype(np.int64)
        total = int(last.sum())
        return last / float(total) if total else np.zeros(len(last))

    @property
    def ranking(self):
        """The labels by prob_all descending, ties by label; None when the last column lumps."""
        return None if self.lumped else np.lexsort((np.arange(len(self.alleles)), -self.carriers[:, -1].astype(np.int64)))


def simuCarriers(pedigree, pro=None, controls=None, simulNo=5000, seed=None, maxCount=None, device=None):
    """gen.simuCarriers(pedigree, pro = pro(pedigree), controls = None, simulNo = 5000): a set of affected probands (the cases, pro)
    carries a rare variant -- which founder allele most probably introduced it, and how many of the cases does one founder allele
    reach?  Every founder allele is dropped down the pedigree under its own label simulNo times (the labels of gen.simuIdentity under
    the same seed), and per simulation and founder allele the distinct cases that carry it are counted, and those that carry it on
    both sides; a simulation in which any of the controls (individuals known not to carry the variant) carries the allele is set
    aside in excluded.  One sweep answers for every founder allele what GENLIB's gen.simuProb answers for one ancestor per call.
    Returns a SimuCarriers: carriers, homozygotes, excluded, at_least(k), mean_carriers, prob_all, prob_all_hom, posterior, ranking.

    The result is a pure function of the pedigree's relations, the SETS of cases and of controls (order and repeats change nothing),
    the seed, simulNo and maxCount (include/genphi.h); gen.branching(pedigree, pro=..) first changes nothing.  maxCount=k keeps the
    columns 0 .. k, the last one holding every count >= k (for many cases: the tables are n_labels x (len(cases) + 1) otherwise).
    seed=None draws 64 fresh bits; pass a seed to repeat a run.  The sweep and the counts run on the GPU (csrc/carry.hip); only
    (2 W + 1) n_labels integers come back.

    KeyError for an unknown ID; ValueError for an individual in both lists, an empty pro, more than 32,767 distinct cases, tables of
    more than 2^31 - 1 cells, simulNo outside 1 .. 2^24 or a negative maxCount.  Each call plans, sweeps and frees its own handle."""
    cases = globals()["pro"](pedigree) if pro is None else np.ascontiguousarray(pro, dtype=np.int64)
    others = np.zeros(0, dtype=np.int64) if controls is None else np.ascontiguousarray(controls, dtype=np.int64)
    h = CarriersPlan(pedigree.ind, pedigree.father, pedigree.mother, cases, others, simul_no=simulNo, seed=seed,
                     max_count=0 if maxCount is None else maxCount)
    try:
        h.compute(device=device)
        excluded = h.excluded_to_host()
        tables = []
        for t in (h.carriers_to_host(), h.homozygotes_to_host()):
            t[:, 0] = h.simul_no - excluded - t[:, 1:].sum(axis=1, dtype=np.int64)
            tables.append(t)
        return SimuCarriers(np.unique(cases), np.unique(others), h.alleles(), tables[0], tables[1], excluded, h.simul_no, h.seed)
    finally:
        h.close()


class SimuOrigins:
    """What gen.simuOrigins returns.  pro: the distinct probands that are in a group, in order of first appearance; alleles: int64
    (n_labels, 2), the ID and the side (0 = from the father) of every founder allele, in label order; names: the groups, sorted
    (["all"] without groups); sizes: int64 (G,), the distinct probands of every group; simulNo and the seed used.  The integer
    tables (the definition is the text of genphi_origin_* in include/genphi.h): copies, autozygous: int64 (G, n_labels); matches:
    int64 (G, G, n_labels), symmetric, [a, a] counting the pairs of DIFFERENT probands of a; autozygous_pro: int32 (len(pro),
    n_labels) with byProband, else None.  Every share below is formed once from the integers, in Float64; a mean over no proband or
    no pair is NaN."""

    def __init__(self, pro, alleles, names, sizes, copies, autozygous, matches, autozygous_pro, simulNo, seed):
        self.pro, self.alleles, self.names, self.sizes = pro, alleles, list(names), np.asarray(sizes, dtype=np.int64)
        self.copies, self.autozygous, self.matches, self.autozygous_pro = copies, autozygous, matches, autozygous_pro
        self.simulNo, self.seed = simulNo, seed

    def __repr__(self):
        return "SimuOrigins(%d probands in %d groups, %d founder alleles, simulNo=%d, seed=%d)" % (len(self.pro), len(self.names), len(self.alleles),
                                                                                                  self.simulNo, self.seed)

    @property
    def founders(self):
        """The IDs of the allele table, ascending: the founders and half-founders of the live set."""
        return np.unique(self.alleles[:, 0])

    def _by_founder(self, table):
        """table (.., n_labels) with the alleles of one founder summed: (.., len(founders))."""
        founders, at = np.unique(self.alleles[:, 0], return_inverse=True)
        out = np.zeros(table.shape[:-1] + (len(founders),), dtype=table.dtype)
        np.add.at(out, (Ellipsis, at), table)
        return out

    @property
    def _pairs(self):
        """int64 (G, G): the pairs of different probands within a group, n_a n_b between two."""
        n = self.sizes
        pairs = np.outer(n, n)
        pairs[np.diag_indices(len(n))] = n * (n - 1) // 2
        return pairs

    @staticmethod
    def _over(num, den):
        """num / den in Float64, NaN where den is 0."""
        den = np.asarray(den, dtype=np.float64)
        return np.divide(num, den, out=np.full(np.broadcast(num, den).shape, np.nan), where=den != 0)

    @property
    def frequency(self):
        """(G, n_labels): the expected frequency of every founder allele among the gene copies of a group, copies / (2 n_a S); a row
        sums to 1."""
        return self._over(self.copies, (2 * self.sizes * self.simulNo)[:, None])

    @property
    def kinship(self):
        """(G, G): the mean kinship within (pairs of different probands) and between groups, the sum over the alleles of matches /
        (4 S pairs): gen.phiMeanGroups' table by gene dropping."""
        return self._over(self.matches.sum(axis=2), 4 * self.simulNo * self._pairs)

    @property
    def kinship_by_allele(self):
        """(G, G, n_labels): the part of kinship that descends from every founder allele; sums to kinship over the last axis."""
        return self._over(self.matches, (4 * self.simulNo * self._pairs)[:, :, None])

    def kinship_by_founder(self):
        """(G, G, len(founders)): kinship_by_allele with the two alleles of a founder summed (from the integers)."""
        return self._over(self._by_founder(self.matches), (4 * self.simulNo * self._pairs)[:, :, None])

    @property
    def share(self):
        """(G, G, n_labels): the share of every founder allele in the kinship of a pair of groups, matches / its sum over the alleles;
        zeros where the pair of groups has no kinship at all."""
        total = self.matches.sum(axis=2)
        return np.divide(self.matches, total[:, :, None], out=np.zeros(self.matches.shape), where=total[:, :, None] != 0)

    @property
    def inbreeding(self):
        """(G,): the mean inbreeding of the probands of every group, the sum over the alleles of autozygous / (n_a S)."""
        return self._over(self.autozygous.sum(axis=1), self.sizes * self.simulNo)

    def inbreeding_by_founder(self):
        """(G, len(founders)): the part of inbreeding that descends from every founder; sums to inbreeding over the last axis."""
        return self._over(self._by_founder(self.autozygous), (self.sizes * self.simulNo)[:, None])

    def partial_inbreeding(self):
        """(len(pro), len(founders)): the partial inbreeding coefficients of every proband (Lacy, Alaks & Walsh 1996): the share of
        the simulations in which both its alleles descend from the founder.  ValueError without byProband."""
        if self.autozygous_pro is None:
            raise ValueError("gen.simuOrigins: partial_inbreeding() needs byProband=True")
        return self._by_founder(self.autozygous_pro.astype(np.int64)) / float(self.simulNo)

    def ranking(self, a, b, k=10):
        """The labels of the k founder alleles with the largest share in the kinship of the groups named a and b (a == b: within
        the group), by larger share and then smaller allele index.  KeyError for an unknown name."""
        for name in (a, b):
            if name not in self.names:
                raise KeyError(name)
        m = self.matches[self.names.index(a), self.names.index(b)]
        return np.lexsort((np.arange(len(m)), -m))[:max(int(k), 0)]


def simuOrigins(pedigree, pro=None, groups=None, simulNo=5000, seed=None, byProband=False, device=None):
    """gen.simuOrigins(pedigree, pro = pro(pedigree), groups = None, simulNo = 5000): which founders does the kinship of the probands
    come from -- within a group, between two groups, and in the inbreeding of the probands themselves (Lacy's partition of kinship and
    inbreeding by founder; the inbreeding half is the partial inbreeding coefficients of Lacy, Alaks & Walsh 1996)?  Every founder
    allele is dropped down the pedigree under its own label simulNo times (the labels of gen.simuIdentity under the same seed), and per
    simulation, founder allele and group the gene copies are counted: k_a copies in group a and k_b in group b are k_a k_b matching
    copy pairs, so no pair of probands is ever looked at.  Returns a SimuOrigins: copies, autozygous, matches, autozygous_pro,
    frequency, kinship, kinship_by_allele, kinship_by_founder(), share, inbreeding, inbreeding_by_founder(), partial_inbreeding(),
    ranking(a, b, k).  Neither GENLIB nor the reference has this function.

    groups: a mapping ID -> group name, as gen._pop returns and gen.simuSegments takes; at most 32 names; probands that are not in it
    are swept (the realisation is that of the whole list) but counted nowhere.  None: one group named "all".  byProband: keep the
    (probands x founder alleles) table that partial_inbreeding() needs.  The result is integers added by integer additions: a pure
    function of the pedigree's relations, the SET of probands with their groups (order and repeats change nothing), the seed and
    simulNo (include/genphi.h); gen.branching(pedigree, pro=..) first changes nothing.  seed=None draws 64 fresh bits; pass a seed to
    repeat a run.  The sweep and the counts run on the GPU (csrc/origin.hip); only the tables come back.  Not offered: origins per pair
    of probands, the exact partial kinship (one kinship sweep per founder), linked loci, more than one device.

    KeyError for an unknown ID; ValueError for an empty pro or groups, no proband in a group, more than 32 groups, more than 32,767
    distinct probands in a group, more than 2^31 - 1 cells with byProband, or simulNo outside 1 .. 2^24.  Each call plans, sweeps and
    frees its own handle."""
    probands = globals()["pro"](pedigree) if pro is None else np.ascontiguousarray(pro, dtype=np.int64)
    if groups is None:
        names, labels = ["all"], None
        grouped = probands
        of = np.zeros(len(probands), dtype=np.int32)
    else:
        if len(groups) == 0:
            raise ValueError("groups is empty")
        names = sorted(set(groups.values()))
        if len(names) > 32:
            raise ValueError("gen.simuOrigins: %d groups: at most 32" % len(names))
        index = {name: k for k, name in enumerate(names)}
        labels = np.array([index[groups[i]] if i in groups else -1 for i in probands.tolist()], dtype=np.int32)
        grouped, of = probands[labels >= 0], labels[labels >= 0]
    h = OriginsPlan(pedigree.ind, pedigree.father, pedigree.mother, probands, labels, n_groups=len(names), simul_no=simulNo, seed=seed,
                    by_proband=byProband)
    try:
        h.compute(device=device)
        first = np.sort(np.unique(grouped, return_index=True)[1])                           # the distinct grouped probands, by first appearance
        sizes = np.bincount(of[first], minlength=len(names)).astype(np.int64)
        G = len(names)
        upper = h.matches_to_host()
        matches = np.zeros((G, G, h.n_labels), dtype=np.int64)
        rows, cols = np.triu_indices(G)                                                     # row-major over the upper triangle
        matches[rows, cols] = upper
        matches[cols, rows] = upper
        return SimuOrigins(grouped[first], h.alleles(), names, sizes, h.copies_to_host(), h.autozygous_to_host(), matches,
                           h.by_proband_to_host() if byProband else None, h.simul_no, h.seed)
    finally:
        h.close()


class SimuUniqueness:
    """What gen.simuUniqueness returns.  pro: the distinct probands, in the order of the rows of the tables (ascending row of the
    plan); n_pop: the distinct probands and others, the population; simulNo and the seed used.  The integer tables (the definition is
    the text of genphi_unique_* in include/genphi.h): alleles, autozygous: int32 (len(pro), K); column min(m, K) - 1 holds the founder
    alleles of the proband that m members of the population carry, K = min(n_pop, maxShare); copies = alleles + autozygous, int64: the
    gene copies, 2 simulNo per proband.  Every share below is formed once from the integers, in Float64."""

    def __init__(self, pro, n_pop, alleles, autozygous, simulNo, seed):
        self.pro, self.n_pop, self.alleles, self.autozygous = pro, int(n_pop), alleles, autozygous
        self.simulNo, self.seed = simulNo, seed
        self.copies = alleles.astype(np.int64) + autozygous.astype(np.int64)
        self.lumped = alleles.shape[1] < self.n_pop

    def __repr__(self):
        return "SimuUniqueness(%d probands in a population of %d, %d columns, simulNo=%d, seed=%d)" % (len(self.pro), self.n_pop, self.alleles.shape[1],
                                                                                                     self.simulNo, self.seed)

    @property
    def uniqueness(self):
        """(len(pro),): MacCluer's genome uniqueness, the probability that a gene copy of the proband is the population's only one
        (with a single column, which lumps every share, it is 1)."""
        return self.copies[:, 0] / (2.0 * self.simulNo)

    @property
    def at_risk(self):
        """(len(pro),): the expected number of founder alleles lost with the proband."""
        return self.alleles[:, 0] / float(self.simulNo)

    @property
    def share_hist(self):
        """(len(pro), K): the share of the proband's gene copies whose allele min(m, K) members of the population carry; a row sums
        to 1."""
        return self.copies / (2.0 * self.simulNo)

    @property
    def mean_share(self):
        """(len(pro),): the mean number of members of the population that carry a gene copy of the proband; None when the last column
        lumps."""
        if self.lumped:
            return None
        return (self.copies @ np.arange(1, self.copies.shape[1] + 1, dtype=np.int64)) / (2.0 * self.simulNo)

    def ranking(self, k=10):
        """The positions in pro of the k probands with the largest uniqueness, by larger uniqueness and then smaller position."""
        return np.lexsort((np.arange(len(self.pro)), -self.copies[:, 0]))[:max(int(k), 0)]


def simuUniqueness(pedigree, pro=None, others=None, simulNo=5000, seed=None, maxShare=8, device=None):
    """gen.simuUniqueness(pedigree, pro = pro(pedigree), others = None, simulNo = 5000): for each proband, how much of what it
    carries is carried by nobody else, and what is lost when it goes -- the genome uniqueness of MacCluer et al. (1986), the statistic
    by which individuals are ranked for breeding, sampling or sequencing.  Every founder allele is dropped down the pedigree under its
    own label simulNo times (the labels of gen.simuIdentity under the same seed); per simulation the members of the population (the
    probands and the others: individuals that count as carriers but are not evaluated) that carry each label are counted, and each
    side of each proband is entered at the share of its label.  Returns a SimuUniqueness: alleles, autozygous, copies, uniqueness,
    at_risk, share_hist, mean_share, ranking(k).  Neither GENLIB nor the reference has this function.

    The result is integers added by integer additions: a pure function of the pedigree's relations, the SETS of probands and of
    others (order and repeats change nothing; an individual in both is a proband), the seed, simulNo and maxShare
    (include/genphi.h); gen.branching(pedigree, pro=..) first changes nothing.  maxShare=k keeps the columns of the shares 1 .. k, the
    last one holding every share >= k; maxShare=0 keeps one column per member of the population.  seed=None draws 64 fresh bits; pass
    a seed to repeat a run.  The sweep and the counts run on the GPU (csrc/unique.hip); only the two tables come back.  Not offered:
    uniqueness within groups, the simulations in which a proband is the sole carrier of at least one allele, linked loci, more than
    one device.

    KeyError for an unknown ID; ValueError for an empty pro, more than 65,535 distinct probands and others, tables of more than
    2^31 - 1 cells, simulNo outside 1 .. 2^24 or a negative maxShare.  Each call plans, sweeps and frees its own handle."""
    probands = globals()["pro"](pedigree) if pro is None else np.ascontiguousarray(pro, dtype=np.int64)
    rest = np.zeros(0, dtype=np.int64) if others is None else np.ascontiguousarray(others, dtype=np.int64)
    h = UniquenessPlan(pedigree.ind, pedigree.father, pedigree.mother, probands, rest, simul_no=simulNo, seed=seed, max_share=maxShare)
    try:
        h.compute(device=device)
        return SimuUniqueness(h.probands(), h.n_pop, h.alleles_to_host(), h.autozygous_to_host(), h.simul_no, h.seed)
    finally:
        h.close()


class SimuSharing:
    """What gen.simuSharing returns.  pro: the listed probands; sums: int64 (N, N, 6), the sums over the simulations of m, m^2, n1,
    n2, g and [n1 > 0] of every pair (include/genphi.h: m = the allele matches summed over the loci, n1 / n2 = the loci with any
    sharing / with both alleles shared, g = the runs of consecutive loci with any sharing); loci, q and probRecomb = q / 65536, the
    recombination probability actually used; simulNo and the seed used; alleles: int64 (n_labels, 2), the ID and the side of every
    founder allele, in label order; labels: int32 (N, 2, simulNo, loci) or None.  Every share below is formed once from the exact
    integers, in Float64."""

    def __init__(self, pro, sums, loci, q, simulNo, seed, alleles, labels):
        self.pro, self.sums, self.loci, self.q, self.simulNo, self.seed, self.alleles, self.labels = pro, sums, loci, q, simulNo, seed, alleles, labels
        self.probRecomb = q / 65536.0

    def __repr__(self):
        return "SimuSharing(%d probands, loci=%d, probRecomb=%g, simulNo=%d, seed=%d)" % (len(self.pro), self.loci, self.probRecomb, self.simulNo,
                                                                                         self.seed)

    @property
    def kinship(self):
        """(N, N): the mean over the simulations of the realised kinship m_s / (4 loci)."""
        return self.sums[..., 0] / float(4 * self.simulNo * self.loci)

    @property
    def kinship_sd(self):
        """(N, N): the standard deviation over the simulations (divisor simulNo) of the realised kinship m_s / (4 loci):
        sqrt(S sum m^2 - (sum m)^2) / (4 S loci), the radicand in exact integers."""
        S = int(self.simulNo)
        m, m2 = self.sums[..., 0], self.sums[..., 1]
        den = 4 * S * self.loci
        if S * int(m2.max(initial=0)) < 2**63:
            num = S * m2 - m * m
            return np.sqrt(num.astype(np.float64)) / float(den)
        num = S * m2.astype(object) - m.astype(object) * m.astype(object)             # Python integers: S sum m^2 may pass 2^63
        return np.sqrt(np.array([float(v) for v in num.ravel()]).reshape(num.shape)) / float(den)

    @property
    def ibd1(self):
        """(N, N): the share of (simulation, locus) at which the pair shares at least one allele identical by descent."""
        return self.sums[..., 2] / float(self.simulNo * self.loci)

    @property
    def ibd2(self):
        """(N, N): the share of (simulation, locus) at which both alleles of the pair are shared."""
        return self.sums[..., 3] / float(self.simulNo * self.loci)

    @property
    def segments(self):
        """(N, N): the mean number of shared segments (runs of consecutive loci with any sharing) per simulation."""
        return self.sums[..., 4] / float(self.simulNo)

    @property
    def segment_loci(self):
        """(N, N): the mean length of a shared segment in loci, sum n1 / sum g; NaN where no segment was seen."""
        g = self.sums[..., 4]
        out = np.full(g.shape, np.nan)
        np.divide(self.sums[..., 2], g, out=out, where=g > 0)
        return out

    @property
    def shared(self):
        """(N, N): the share of the simulations in which the pair shares anything at all."""
        return self.sums[..., 5] / float(self.simulNo)

    @property
    def inbreeding(self):
        """(N,): from the diagonal, (m_ii - 2 S loci) / (2 S loci): the share of (simulation, locus) at which the two alleles of
        proband i are identical by descent."""
        n = np.arange(len(self.pro))
        half = 2 * self.simulNo * self.loci
        return (self.sums[n, n, 0] - half) / float(half)


def sharing_q(loci, length=1.0, probRecomb=None):
    """q of gen.simuSharing: round(65536 probRecomb), or from Haldane's map over loci - 1 equal intervals of a chromosome of `length`
    Morgans, r = (1 - exp(-2 length / (loci - 1))) / 2 (one locus: no interval, q = 0).  ValueError outside 0 .. 32768."""
    if probRecomb is None:
        loci, length = int(loci), float(length)
        if not length >= 0.0:
            raise ValueError("gen.simuSharing: length = %r Morgans" % (length,))
        r = 0.5 * (1.0 - np.exp(-2.0 * length / (loci - 1))) if loci > 1 else 0.0
    else:
        r = float(probRecomb)
    q = int(round(65536.0 * r)) if np.isfinite(r) else -1
    if not 0 <= q <= _capi.GENPHI_LINK_MAX_Q:
        raise ValueError("gen.simuSharing: a recombination probability of %r between neighbouring loci is outside 0 .. 1/2" % (r,))
    return q


def simuSharing(pedigree, pro=None, loci=1024, length=1.0, probRecomb=None, simulNo=1000, seed=None, labels=False, device=None):
    """gen.simuSharing(pedigree, pro = pro(pedigree), loci = 1024, length = 1.0, simulNo = 1000): gene dropping along a chromosome
    of `loci` linked loci (GENLIB's gen.simuHaplo is the model): every founder allele is dropped under its own label, a meiosis
    copies a mosaic of the parent's two chromosomes with crossovers between neighbouring loci, and for every pair of probands the
    loci shared identical by descent are counted in every simulation.  Returns a SimuSharing: sums, and from them kinship,
    kinship_sd (how much the realised kinship varies around it), ibd1, ibd2, segments, segment_loci, shared, inbreeding.

    length is the chromosome's length in Morgans: the recombination probability between neighbours comes from Haldane's map over
    loci - 1 equal intervals; or pass probRecomb itself.  Either is rounded to q / 65536 (sharing_q), and the result reports the
    probRecomb actually used.  The result is a pure function of the pedigree's relations, the probands, loci, q, the seed and
    simulNo (include/genphi.h); a sub-list of probands gives the sub-block and gen.branching(pedigree, pro=..) first changes
    nothing.  seed=None draws 64 fresh bits.  labels=True also returns the probands' labels, (N, 2, simulNo, loci).  The sweep and
    the pair sums run on the GPU (csrc/link.hip).

    KeyError for an unknown ID; ValueError for loci outside 1 .. 4096, a recombination probability outside 0 .. 1/2, simulNo outside
    1 .. 2^24, an empty pro, or 2^31 or more ordered pairs.  Each call plans, sweeps and frees its own handle."""
    probands = globals()["pro"](pedigree) if pro is None else np.ascontiguousarray(pro, dtype=np.int64)
    if not 1 <= int(loci) <= _capi.GENPHI_LINK_MAX_LOCI:
        raise ValueError("gen.simuSharing: loci = %r is outside 1 .. 4096" % (loci,))
    q = sharing_q(loci, length, probRecomb)
    h = SharingPlan(pedigree.ind, pedigree.father, pedigree.mother, probands, loci=loci, q=q, simul_no=simulNo, seed=seed, labels=labels)
    try:
        h.compute(device=device)
        return SimuSharing(probands, h.sums_to_host(), h.loci, h.q, h.simul_no, h.seed, h.alleles(), h.labels_to_host() if labels else None)
    finally:
        h.close()


class SimuSegments:
    """What gen.simuSegments returns.  pro: the listed probands; edges: int32, the bin edges in loci (a segment of len loci is in
    bin b when edges[b] <= len < edges[b + 1]); minLoci; counts, loci_in, censored: int64 (n_bins,), or (G, G, n_bins) and symmetric
    with groups -- the segments of every bin over the pairs i < j of list positions and all simulations, the loci in them, and those
    of them that the end of the chromosome cut short (they hold locus 0 or the last locus); below, above: the same three integers
    (segments, loci, censored) for the lengths under edges[0] and at or above edges[-1], int64 (3,) or (G, G, 3); names (sorted) and
    sizes (list positions per group) with groups, else None; pairs: int64 (N, N, 3), per pair the sums over the simulations of the
    segments of at least minLoci loci, of the loci in them, and of the longest segment; sharing: the SimuSharing of the same run.
    Every property is formed once from the exact integers, in Float64."""

    def __init__(self, pro, edges, minLoci, hist, pairs, sharing, names=None, sizes=None):
        self.pro, self.edges, self.minLoci, self.pairs, self.sharing, self.names, self.sizes = pro, edges, minLoci, pairs, sharing, names, sizes
        table = hist if names is not None else hist[0, 0]
        self.counts = np.ascontiguousarray(table[..., 1:-1, 0])
        self.loci_in = np.ascontiguousarray(table[..., 1:-1, 1])
        self.censored = np.ascontiguousarray(table[..., 1:-1, 2])
        self.below = np.ascontiguousarray(table[..., 0, :])
        self.above = np.ascontiguousarray(table[..., -1, :])

    def __repr__(self):
        upper = np.triu(np.ones(self.counts.shape[:2], dtype=bool)) if self.names is not None else None
        total = int(self.counts.sum() + self.below[..., 0].sum() + self.above[..., 0].sum()) if upper is None else int(
            self.counts[upper].sum() + self.below[upper][:, 0].sum() + self.above[upper][:, 0].sum())
        return "SimuSegments(%d probands, loci=%d, simulNo=%d, %d bins over [%d, %d), %d segments%s)" % (
            len(self.pro), self.sharing.loci, self.sharing.simulNo, len(self.edges) - 1, self.edges[0], self.edges[-1], total,
            "" if self.names is None else ", %d groups" % len(self.names))

    @property
    def mean_length(self):
        """Per bin: the mean length in loci of its segments, loci_in / counts; NaN where the bin is empty."""
        out = np.full(self.counts.shape, np.nan)
        np.divide(self.loci_in, self.counts, out=out, where=self.counts > 0)
        return out

    @property
    def segments_over(self):
        """(N, N): the mean number per simulation of the pair's segments of at least minLoci loci."""
        return self.pairs[..., 0] / float(self.sharing.simulNo)

    @property
    def loci_over(self):
        """(N, N): the mean number per simulation of the pair's loci in segments of at least minLoci loci."""
        return self.pairs[..., 1] / float(self.sharing.simulNo)

    @property
    def longest(self):
        """(N, N): the mean over the simulations of the pair's longest segment in loci (0 in a simulation without sharing)."""
        return self.pairs[..., 2] / float(self.sharing.simulNo)

    @property
    def locus_cM(self):
        """The genetic length of the interval between neighbouring loci in centimorgans, -50 ln(1 - 2 q / 65536): Haldane's map
        read backwards from the recombination probability actually used; infinite for independent loci (q = 32768)."""
        with np.errstate(divide="ignore"):
            return float(-50.0 * np.log(np.float64(1.0 - 2.0 * self.sharing.q / 65536.0)))


def _segment_edges(bins, loci):
    if bins is None:
        top = 1
        while top <= loci:
            top *= 2
        edges = [1]
        while edges[-1] < top:
            edges.append(edges[-1] * 2)                  # 1, 2, 4, .. up to and including the first power of two above loci
        edges[-1] = min(edges[-1], _capi.GENPHI_SEG_MAX_EDGE)     # loci = 4096: 8192 is no edge; the last bin is [4096, 4097)
        return np.array(edges, dtype=np.int32)
    return _capi._i32_list(bins, "bins")


def simuSegments(pedigree, pro=None, loci=1024, length=1.0, probRecomb=None, simulNo=1000, seed=None, bins=None, minLoci=1, groups=None,
                 device=None):
    """gen.simuSegments(pedigree, pro = pro(pedigree), loci = 1024, length = 1.0, simulNo = 1000): the length spectrum of the
    segments that pairs of probands share identical by descent, by gen.simuSharing's gene dropping along a chromosome of `loci`
    linked loci.  A segment is a maximal run of consecutive loci at which the pair shares an allele (what SimuSharing.segments
    counts); its length is a number of loci, locus_cM centimorgans each.  Returns a SimuSegments: the histogram of the lengths over
    all pairs i < j and all simulations (counts, loci_in, censored per bin, below and above), with `groups` within and between
    sub-populations, and per pair the segments of at least minLoci loci (segments_over, loci_over) and the longest (longest).
    Neither GENLIB nor the reference has this function.

    pedigree, pro, loci, length, probRecomb, simulNo and seed are gen.simuSharing's, and .sharing is the SimuSharing of the same
    run.  bins: None = the edges 1, 2, 4, .. up to and including the first power of two above loci (at loci = 4096 that would be
    8192, past the largest edge: the list ends 2048, 4096, 4097, so the last bin holds the whole chromosome and `above` stays
    empty, as for every other loci); or the edges themselves, 2 ..
    257 strictly increasing integers in 1 .. 4097.  minLoci: 1 .. 4097.  groups: a mapping ID -> group name, as gen._pop returns
    and gen.phiHist takes; probands that are not in it take part in no count of the histogram (they keep their per-pair sums); at
    most 32 groups and G (G + 1) / 2 x (bins + 2) <= 2,048.  The result is integers added by integer additions: a pure function of
    the pedigree's relations, the probands, loci, q, the seed, simulNo, the edges, minLoci and the groups.  The sweep, the pair sums
    and the segment walk run on the GPU (csrc/link.hip).

    KeyError and ValueError as gen.simuSharing; ValueError for edges, minLoci or groups outside the limits."""
    probands = globals()["pro"](pedigree) if pro is None else np.ascontiguousarray(pro, dtype=np.int64)
    if not 1 <= int(loci) <= _capi.GENPHI_LINK_MAX_LOCI:
        raise ValueError("gen.simuSegments: loci = %r is outside 1 .. 4096" % (loci,))
    q = sharing_q(loci, length, probRecomb)
    edges = _segment_edges(bins, int(loci))
    names = labels = sizes = None
    if groups is not None:
        if len(groups) == 0:
            raise ValueError("groups is empty")
        names = sorted(set(groups.values()))
        index = {name: k for k, name in enumerate(names)}
        labels = np.array([index[groups[i]] if i in groups else -1 for i in probands.tolist()], dtype=np.int32)
        if len(names) > _capi.GENPHI_SEG_MAX_GROUPS:
            raise ValueError("gen.simuSegments: %d groups: at most %d" % (len(names), _capi.GENPHI_SEG_MAX_GROUPS))
        sizes = np.bincount(labels[labels >= 0], minlength=len(names)).astype(np.int64)
    h = SharingPlan(pedigree.ind, pedigree.father, pedigree.mother, probands, loci=loci, q=q, simul_no=simulNo, seed=seed)
    try:
        h.request_segments(edges, min_loci=minLoci, groups=labels)
        h.compute(device=device)
        hist, pairs = h.segments_to_host()
        if names is not None and hist.shape[0] < len(names):                              # the last names have no listed proband
            full = np.zeros((len(names), len(names)) + hist.shape[2:], dtype=np.int64)
            full[:hist.shape[0], :hist.shape[0]] = hist
            hist = full
        sharing = SimuSharing(probands, h.sums_to_host(), h.loci, h.q, h.simul_no, h.seed, h.alleles(), None)
        return SimuSegments(probands, edges, int(minLoci), hist, pairs, sharing, names, sizes)
    finally:
        h.close()


def depth(pedigree):
    """gen.depth(pedigree) (src/describe.jl:43-66): the number of generations of the pedigree, 1 + the longest ascent of any
    individual (1 for a pedigree of founders, 0 for an empty one).  One linear pass on the host (csrc/loader.cpp) where the
    reference recurses without memory; there is no arithmetic worth a kernel launch."""
    return _capi.genealogy_depth(pedigree.ind, pedigree.father, pedigree.mother)


def nomen(pedigree):
    """gen.nomen(pedigree): the number of men, sex == 1 (src/describe.jl:6-14)."""
    return int(np.count_nonzero(pedigree.sex == 1))


def nowomen(pedigree):
    """gen.nowomen(pedigree): the number of women, sex == 2 (src/describe.jl:21-29)."""
    return int(np.count_nonzero(pedigree.sex == 2))


def noind(pedigree):
    """gen.noind(pedigree): the number of individuals (src/describe.jl:36)."""
    return len(pedigree)


def _id_list(IDs):
    return np.atleast_1d(np.asarray(IDs, dtype=np.int64)).ravel()


def ancestor(pedigree, IDs):
    """gen.ancestor(pedigree, ID) / gen.ancestor(pedigree, IDs) (src/identify.jl:164-199): the ancestors of one individual, or of
    several (the union), ascending.  Strict: an individual is not its own ancestor.  Host only (csrc/loader.cpp).  KeyError for an
    unknown ID."""
    return _capi.ancestors(pedigree.ind, pedigree.father, pedigree.mother, _id_list(IDs))


def descendant(pedigree, IDs):
    """gen.descendant(pedigree, ID) / gen.descendant(pedigree, IDs) (src/identify.jl:203-215): the descendants of one individual, or
    of several (the union), ascending.  Strict: an individual is not its own descendant.  Host only (csrc/loader.cpp).  KeyError for
    an unknown ID."""
    return _capi.descendants(pedigree.ind, pedigree.father, pedigree.mother, _id_list(IDs))


def children(pedigree, ID):
    """gen.children(pedigree, ID) (src/identify.jl:77-80): the children of an individual, ascending.  Host only (csrc/loader.cpp).
    KeyError for an unknown ID."""
    return _capi.children(pedigree.ind, pedigree.father, pedigree.mother, int(ID))


_MRCA_CANDIDATE_SEARCHES = 16          # ancestor sets looked at for the shortest candidate list (any one of them is a valid list)


def _common_ancestors(pedigree, IDs, device):
    """The individuals that are a strict ancestor of every one of IDs, ascending.  The common set lies inside the ancestors of any
    single ID: the smallest such set among the first few IDs is the candidate list, and gen.rec (strict, distinct probands) counts,
    per candidate, how many of the IDs descend from it."""
    pedigree.positions(IDs)                                        # KeyError on an unknown ID (gen.rec ignores them)
    distinct = np.unique(IDs)
    if len(distinct) == 0:
        return np.zeros(0, dtype=np.int64)
    candidates = min((ancestor(pedigree, [i]) for i in distinct[:_MRCA_CANDIDATE_SEARCHES]), key=len)
    if len(candidates) == 0:
        return candidates
    return candidates[rec(pedigree, distinct, candidates, device=device) == len(distinct)]


def findFounders(pedigree, IDs, device=None):
    """gen.findFounders(pedigree, IDs) (src/identify.jl:83-95): the founders from whom every one of IDs descends, ascending.  A
    founder listed in IDs is not its own ancestor.  KeyError for an unknown ID."""
    common = _common_ancestors(pedigree, _id_list(IDs), device)
    pos = pedigree.positions(common)
    return common[(pedigree.father[pos] == 0) & (pedigree.mother[pos] == 0)]


class GenMatrix:
    """The reference's GenMatrix (src/identify.jl:129-133): meioses[i, j] between individuals[i] (rows) and ancestors[j] (columns)."""

    def __init__(self, individuals, ancestors, meioses):
        self.individuals, self.ancestors, self.meioses = individuals, ancestors, meioses

    def __repr__(self):
        return "GenMatrix(individuals=%r, ancestors=%r, meioses=%r)" % (self.individuals.tolist(), self.ancestors.tolist(), self.meioses.tolist())


def findMRCA(pedigree, IDs, device=None):
    """gen.findMRCA(pedigree, IDs) (src/identify.jl:97-160): the most recent common ancestors (MRCAs) of IDs and the meioses
    between each individual and each of them, as a GenMatrix: `individuals` = IDs as given (a repeated ID repeats its row),
    `ancestors` ascending, `meioses` int64 of shape (len(IDs), len(ancestors)).

    The common ancestors come from gen.rec over the ancestors of one of the IDs, the MRCAs are the common ancestors without a
    common child (csrc/loader.cpp: equal to the reference's setdiff with the ancestors of the common set), and the distances are
    one gen.meioses sweep (csrc/dist.hip) where the reference enumerates every ascending path per pair.  KeyError for an unknown
    ID.  One deviation: for individuals without any common ancestor the reference (as far as its source reads; not run) calls
    union() without arguments and throws; here the GenMatrix has no ancestors and a (len(IDs), 0) matrix."""
    IDs = _id_list(IDs)
    common = _common_ancestors(pedigree, IDs, device)
    mrcas = _capi.mrca_filter(pedigree.ind, pedigree.father, pedigree.mother, common)
    if len(mrcas) == 0 or len(IDs) == 0:
        return GenMatrix(IDs, mrcas, np.zeros((len(IDs), len(mrcas)), dtype=np.int64))
    return GenMatrix(IDs, mrcas, meioses(pedigree, IDs, mrcas, device=device).astype(np.int64))


def findDistance(pedigree, IDs, ancestorID, device=None):
    """gen.findDistance(pedigree, IDs, ancestorID) (src/describe.jl:291-300): the meioses between IDs[0] and IDs[1] through
    ancestorID, that is, the sum of their shortest ascents to it (only the first two IDs are used; IndexError with fewer).  An ID
    equal to ancestorID is at distance 0.  ValueError when ancestorID is not an ancestor of both (the reference takes the minimum
    of an empty vector and throws); KeyError for an unknown ID."""
    IDs = _id_list(IDs)
    if len(IDs) < 2:
        raise IndexError("findDistance needs two IDs, got %d" % len(IDs))
    d = meioses(pedigree, IDs[:2], [int(ancestorID)], device=device)[:, 0]
    if np.any(d < 0):
        raise ValueError("%d is not an ancestor of %d" % (int(ancestorID), int(IDs[:2][d < 0][0])))
    return int(d[0]) + int(d[1])


def _findMinDistanceMRCA(pedigree, IDs, device=None):
    """gen._findMinDistanceMRCA(pedigree, IDs) (src/identify.jl:105-114): the smallest findDistance of the first two IDs over the
    MRCAs of all IDs.  ValueError without an MRCA; IndexError with fewer than two IDs."""
    IDs = _id_list(IDs)
    if len(IDs) < 2:
        raise IndexError("_findMinDistanceMRCA needs two IDs, got %d" % len(IDs))
    m = findMRCA(pedigree, IDs, device=device)
    if len(m.ancestors) == 0:
        raise ValueError("the individuals have no common ancestor")
    return int((m.meioses[0] + m.meioses[1]).min())


def sparse_phi(pedigree, probandIDs=None, device=None):
    """gen.sparse_phi(pedigree, probandIDs = pro(pedigree)) (src/compute.jl:321-447): the reference's
    queue-driven kinship algorithm, returning a KinshipMatrix indexed by proband IDs (`K[1, 2]`,
    `repr(K)` = the reference's `show` line, `gen.phiMean(K)`).  Computed on the GPU one depth at a
    time on a dense active matrix (csrc/sparse_phi.hip); values, lookup behaviour and the number of
    stored entries are the reference's.  KeyError for an unknown proband ID."""
    probandIDs = pro(pedigree) if probandIDs is None else np.asarray(probandIDs, dtype=np.int64)
    return KinshipMatrix(pedigree.ind, pedigree.father, pedigree.mother, probandIDs, device=device)


def phiMean(phi_matrix):
    """gen.phiMean(::Matrix{Float32}) (src/compute.jl:454-459): mean off-diagonal kinship of a host
    matrix, accumulated in float32 like the reference.  numpy's float32 pairwise summation blocks
    differently from Julia's `sum`, so on large matrices the last bits can differ (about 1 ulp of
    Float32; exact whenever the sums are exact, e.g. 0.171875 on geneaJi, test/runtests.jl:53).
    `PhiPlan.phi_mean()` reduces the RESIDENT matrix on the device instead (Float64 accumulation,
    one rounding; no 40 GB device-to-host copy at N = 1e5)."""
    if isinstance(phi_matrix, KinshipMatrix):            # phiMean(::KinshipMatrix), src/compute.jl:467-472
        nr, _, total, diagonal = phi_matrix.info()
        return np.float32((total - diagonal) / (nr * (nr - 1) / 2))
    m = np.asarray(phi_matrix, dtype=np.float32)
    total = np.float32(m.sum(dtype=np.float32))
    diagonal = np.float32(np.diagonal(m).sum(dtype=np.float32))
    total = np.float32(total - diagonal)
    return np.float32(total / np.float32(m.size - m.shape[0]))


def _pop(filename):
    """gen._pop(filename) (src/GenLib.jl:76-92): the population of each proband as a dict ID -> name, from a file with a header
    line and two whitespace-separated fields per line (the reference's pop140.csv)."""
    population = {}
    with open(filename) as file:
        next(file, None)
        for line in file:
            ind, name = line.split()
            population[int(ind)] = name
    return population


def _group_order(groups, probandIDs=None):
    """Host side of gen.phiMeanGroups: (names, IDs, labels).  names = the group names, sorted; IDs = the probands (each once) ordered
    by (group name, ID), those in no group last; labels[i] = index in names of the group of IDs[i], -1 = in no group.  In this order
    every group is one run, which is the form genphi_result_group_sums reads without a column table."""
    if len(groups) == 0:
        raise ValueError("groups is empty")
    names = sorted(set(groups.values()))
    index = {name: k for k, name in enumerate(names)}
    ids = np.unique(np.fromiter(groups.keys(), dtype=np.int64, count=len(groups)) if probandIDs is None else np.asarray(probandIDs, dtype=np.int64))
    labels = np.array([index[groups[i]] if i in groups else -1 for i in ids.tolist()], dtype=np.int32)
    key = np.where(labels < 0, len(names), labels)
    order = np.argsort(key, kind="stable")                 # (ids ascend already)
    return names, ids[order], labels[order]


class GroupMeans:
    """What gen.phiMeanGroups returns: `names` (sorted), `sizes` (probands per group) and `mean`, the float64 table of mean kinships
    (mean[a, a] within names[a], off-diagonal pairs only; mean[a, b] between names[a] and names[b]; NaN where there is no pair)."""

    def __init__(self, names, sizes, mean):
        self.names, self.sizes, self.mean = names, sizes, mean

    def __repr__(self):
        width = max(len(str(n)) for n in self.names)
        lines = ["GroupMeans of %d groups (mean kinship within, on the diagonal, and between groups):" % len(self.names)]
        for a, name in enumerate(self.names):
            lines.append("%-*s n=%-6d %s" % (width, name, self.sizes[a], " ".join("%.6f" % v for v in self.mean[a])))
        return "\n".join(lines)


def phiMeanGroups(pedigree, groups, probandIDs=None, device=None):
    """Mean kinship within and between groups of probands, e.g. the populations of gen._pop(pop140.csv): phiMean
    (src/compute.jl:454-459) of every diagonal block of gen.phi and the plain mean of every other block, reduced on the device
    from the resident matrix, which is never copied (genphi_result_group_sums; one pass over it).

    groups: a mapping ID -> group name (any hashable, sortable value).  probandIDs: the probands of the sweep, by default the
    keys of groups; IDs that are not in groups take part in the sweep but belong to no group.  Returns a GroupMeans.
    KeyError for an unknown ID, ValueError for an empty groups."""
    names, ids, labels = _group_order(groups, probandIDs)
    pedigree.positions(ids)                                 # KeyError on an unknown ID
    pl, key = _plan_for(pedigree, ids, device)
    keep = False
    try:
        pl.compute_device(device=device)
        sums, diag, _, sizes, _ = pl.group_sums(labels, len(names))
        keep = key is not None and _keep_plan(pedigree, key, pl, ids)
    finally:
        if not keep:
            if key is not None and key in pedigree._plans and pedigree._plans[key][0] is pl:
                del pedigree._plans[key]
            pl.close()
    return GroupMeans(names, sizes, _capi.mean_from_group_sums(sums, diag, sizes))


class PhiOver:
    """What gen.phiOver returns: the pairs of probands whose kinship is at or above the threshold, as parallel arrays sorted by
    `row`, then `col`: `row` < `col` (int32, 0-based positions in the order of the probands), `pro1` / `pro2` (int64 IDs of those
    positions, None when no IDs were given with a host matrix) and `kinship` (float32, the matrix entries bit for bit)."""

    def __init__(self, threshold, row, col, pro1, pro2, kinship):
        self.threshold, self.row, self.col, self.pro1, self.pro2, self.kinship = threshold, row, col, pro1, pro2, kinship

    def __len__(self):
        return len(self.row)

    def __repr__(self):
        lines = ["PhiOver: %d pairs with kinship >= %g" % (len(self), self.threshold)]
        for k in range(min(len(self), 5)):
            a, b = (self.row[k], self.col[k]) if self.pro1 is None else (self.pro1[k], self.pro2[k])
            lines.append("%d %d %.6g" % (a, b, self.kinship[k]))
        if len(self) > 5:
            lines.append("...")
        return "\n".join(lines)


def phiOver(x, threshold, probandIDs=None, device=None):
    """GENLIB's gen.phiOver(phiMatrix, threshold): the pairs of probands related at or above `threshold`.  Returns a PhiOver.

    x a Pedigree: gen.phi's sweep for probandIDs (default gen.pro), then the selection on the device from the resident matrix,
    which is never copied (genphi_result_over; two passes over its upper triangle).  x a host matrix (GENLIB's own
    signature): the same selection in numpy on its strict upper triangle; pro1 / pro2 come from probandIDs if given.

    The definition is this package's own: a pair (i, j) is listed when i < j and float64(Phi[i, j]) >= threshold, each pair
    once, in row-major order, with 0-based positions (duplicate probandIDs collapsed, as gen.phi does).  GENLIB's R function could
    not be consulted when this was written: its column names and its 1-based `line` / `column` are not reproduced.
    ValueError for a NaN threshold, KeyError for an unknown proband ID."""
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("the threshold is NaN")
    if isinstance(x, Pedigree):
        ids = pro(x) if probandIDs is None else np.ascontiguousarray(probandIDs, dtype=np.int64)
        x.positions(ids)                                        # KeyError on an unknown ID
        pl, key = _plan_for(x, ids, device)
        keep = False
        try:
            pl.compute_device(device=device)
            row, col, val = pl.phi_over(threshold)
            keep = key is not None and _keep_plan(x, key, pl, ids)
        finally:
            if not keep:
                if key is not None and key in x._plans and x._plans[key][0] is pl:
                    del x._plans[key]
                pl.close()
        _, first = np.unique(ids, return_index=True)
        ids = ids[np.sort(first)]                               # duplicates collapse: first occurrences, in order
        return PhiOver(threshold, row, col, ids[row], ids[col], val)
    m = np.asarray(x, dtype=np.float32)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError("gen.phiOver takes a Pedigree or a square kinship matrix, got shape %s" % (m.shape,))
    ids = None if probandIDs is None else np.asarray(probandIDs, dtype=np.int64)
    if ids is not None and ids.shape != (len(m),):
        raise ValueError("probandIDs must name the %d rows of the matrix" % len(m))
    row, col = np.nonzero(np.triu(m.astype(np.float64) >= threshold, 1))
    row, col = row.astype(np.int32), col.astype(np.int32)
    return PhiOver(threshold, row, col, None if ids is None else ids[row], None if ids is None else ids[col], m[row, col])


class PhiClusters:
    """What gen.phiClusters returns: the connected components of the graph whose edges are the pairs of probands with kinship >=
    `threshold`.  `pro` (int64, the N IDs in the order of the rows, None when no IDs were given with a host matrix), `label` (int32
    (N,), the smallest 0-based position in each proband's cluster), `cluster` (int32 (N,), dense numbers 0 .. K - 1 in the order of
    each cluster's first member), `sizes` (int64 (K,)) and `n_pairs` (the number of edges; None when the clusters were cut from a gen.phiTree, which never counts
    them)."""

    def __init__(self, threshold, pro, label, n_pairs):
        self.threshold, self.pro, self.label, self.n_pairs = threshold, pro, label, None if n_pairs is None else int(n_pairs)
        first = np.flatnonzero(label == np.arange(len(label), dtype=np.int64))      # the first member of every cluster, ascending
        number = np.zeros(len(label), dtype=np.int32)
        number[first] = np.arange(len(first), dtype=np.int32)
        self.cluster = number[label] if len(label) else number
        self.sizes = np.bincount(self.cluster, minlength=len(first)).astype(np.int64)

    def __len__(self):
        return len(self.sizes)

    def members(self, k):
        """The probands of cluster k, in order: their IDs, or their positions when there are no IDs."""
        if not 0 <= int(k) < len(self.sizes):
            raise IndexError("cluster %d of %d" % (int(k), len(self.sizes)))
        pos = np.flatnonzero(self.cluster == int(k)).astype(np.int32)
        return pos if self.pro is None else self.pro[pos]

    def __repr__(self):
        pairs = "pairs not counted" if self.n_pairs is None else "%d pairs" % self.n_pairs       # (None: cut from a gen.phiTree)
        return "PhiClusters: %d probands in %d clusters at kinship >= %g (%s), the largest of %d" % (
            len(self.label), len(self.sizes), self.threshold, pairs, int(self.sizes.max()) if len(self.sizes) else 0)


class PhiUnrelated:
    """What gen.phiUnrelated returns: a maximal set of probands no two of which have kinship >= `threshold`.  `pro` (int64, the N
    IDs in the order of the rows, None when no IDs were given with a host matrix), `keep` (bool (N,)), `index` (int32, the positions
    kept, ascending), `kept` (their IDs, None without `pro`), `degree` (int32 (N,), each proband's number of relatives at or above
    the threshold) and `rounds` (the launches the device took; 0 for a host matrix)."""

    def __init__(self, threshold, pro, keep, degree, rounds):
        self.threshold, self.pro, self.keep, self.degree, self.rounds = threshold, pro, keep, degree, int(rounds)
        self.index = np.flatnonzero(keep).astype(np.int32)
        self.kept = None if pro is None else pro[self.index]

    def __len__(self):
        return len(self.index)

    def __repr__(self):
        return "PhiUnrelated: %d of %d probands kept, no two with kinship >= %g (%d rounds)" % (
            len(self.index), len(self.keep), self.threshold, self.rounds)


def _threshold(threshold):
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("the threshold is NaN")
    return threshold


def phiClusters(x, threshold, probandIDs=None, device=None):
    """The families at a kinship cutoff: the connected components of the graph whose edges are the pairs of probands with
    float64(Phi[i, j]) >= threshold (gen.phiOver's rule; never the diagonal).  Returns a PhiClusters.  Neither GENLIB nor the
    reference has this function.

    x a Pedigree: gen.phi's sweep for probandIDs (default gen.pro; duplicates collapse, as gen.phi does), then a lock-free
    union-find on the device over one read of the upper triangle of the resident matrix, which is never copied and whose pairs are
    never listed (genphi_result_clusters).  x a square host matrix: the same answer in numpy and a plain loop (its
    upper triangle decides); `pro` comes from probandIDs if given.  ValueError for a NaN threshold, KeyError for an unknown
    proband ID."""
    threshold = _threshold(threshold)
    if isinstance(x, Pedigree):
        ids, (label, n_pairs) = _resident_query(x, probandIDs, device, lambda pl: pl.clusters(threshold))
        return PhiClusters(threshold, ids, label, n_pairs)
    m, ids = _host_matrix(x, probandIDs, "gen.phiClusters")
    a = np.triu(m >= threshold, 1)
    n_pairs = int(np.count_nonzero(a))
    a = a | a.T
    label = np.full(len(m), -1, dtype=np.int32)
    for s in range(len(m)):                                     # ascending: the first unlabelled position is its cluster's smallest
        if label[s] >= 0:
            continue
        label[s] = s
        stack = [s]
        while stack:
            fresh = np.flatnonzero(a[stack.pop()] & (label < 0))
            label[fresh] = s
            stack.extend(fresh.tolist())
    return PhiClusters(threshold, ids, label, n_pairs)


def phiUnrelated(x, threshold, priority=None, probandIDs=None, device=None):
    """A maximal set of probands no two of which are related at or above `threshold` -- the "kinship cutoff" of association studies,
    allele-frequency estimates and founder-population sampling.  Returns a PhiUnrelated.  Neither GENLIB nor the reference has
    this function.

    Two probands i != j are related when float64(Phi[i, j]) >= threshold (gen.phiOver's rule).  The set is the answer of the
    sequential greedy rule: visit the probands in ascending order of (priority[i], i) and keep one iff none of its relatives has
    been kept.  priority: None or "degree" -- the number of relatives, so the fewest relatives first, the usual heuristic for a large
    set; "position" -- all equal, so earlier probands win; or N integers in the int32 range, smaller is kept first.  The answer is
    unique given the matrix, the threshold and the priorities.

    x a Pedigree: gen.phi's sweep for probandIDs (default gen.pro; duplicates collapse, as gen.phi does; an array of priorities
    names the collapsed probands), then rounds over the rows of the resident matrix on the device, which is never copied and whose
    pairs are never listed (genphi_result_unrelated).  x a square host matrix: the same answer in numpy and a plain
    loop (its upper triangle decides).  ValueError for a NaN threshold, a priority of the wrong length or not of integers; KeyError
    for an unknown proband ID."""
    threshold = _threshold(threshold)
    if isinstance(priority, str):
        if priority not in ("degree", "position"):
            raise ValueError("gen.phiUnrelated: priority %r: \"degree\", \"position\" or one integer per proband" % (priority,))
    by_degree = priority is None or (isinstance(priority, str) and priority == "degree")

    def priorities(n):
        if by_degree:
            return None
        if isinstance(priority, str):
            return np.zeros(n, dtype=np.int32)
        return _capi.as_priority(priority, n)

    if isinstance(x, Pedigree):
        ids, (keep, degree, rounds) = _resident_query(x, probandIDs, device, lambda pl: pl.unrelated(threshold, priorities(pl.n_probands)))
        return PhiUnrelated(threshold, ids, keep, degree, rounds)
    m, ids = _host_matrix(x, probandIDs, "gen.phiUnrelated")
    n = len(m)
    pri = priorities(n)
    a = np.triu(m >= threshold, 1)
    a = a | a.T
    degree = a.sum(axis=1).astype(np.int32)
    keep, barred = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for i in np.lexsort((np.arange(n), degree if pri is None else pri)):      # ascending (priority, position)
        if not barred[i]:
            keep[i] = True
            barred |= a[i]
    return PhiUnrelated(threshold, ids, keep, degree, 0)


class PhiTree:
    """What gen.phiTree returns: the single-linkage tree of the kinships, as the M = N - n_trees edges of the maximum spanning forest
    of the graph whose edges are the pairs with kinship >= `floor`, ordered by larger kinship first, then smaller row, then smaller
    column.  `pro` (int64, the N IDs in the order of the rows, None when no IDs were given with a host matrix), `row`, `col` (int32
    (M,), 0-based positions, row < col), `pro1`, `pro2` (the IDs at those positions, None without `pro`), `kinship` (float32 (M,),
    the matrix entries bit for bit), `floor`, `n_trees` (the clusters at `floor`) and `rounds` (the rounds the device took; 0 for a
    host matrix).  len() is the number of edges."""

    def __init__(self, floor, pro, n, row, col, kinship, n_trees, rounds):
        self.floor, self.pro, self.n, self.row, self.col, self.kinship = floor, pro, int(n), row, col, kinship
        self.n_trees, self.rounds = int(n_trees), int(rounds)
        self.pro1 = None if pro is None else pro[row]
        self.pro2 = None if pro is None else pro[col]

    def __len__(self):
        return len(self.row)

    def __repr__(self):
        top = " from %g" % float(self.kinship[0]) if len(self.row) else ""
        return "PhiTree: %d probands, %d edges%s down to kinship >= %g, %d tree%s (%d rounds)" % (
            self.n, len(self.row), top, self.floor, self.n_trees, "" if self.n_trees == 1 else "s", self.rounds)

    def _passing(self, t):
        """The edges with float64(kinship) >= t are the first k of the list: k."""
        t = _threshold(t)
        if t < self.floor:
            raise ValueError("PhiTree: the tree was built down to kinship %g and says nothing about %g" % (self.floor, t))
        return int(np.count_nonzero(self.kinship.astype(np.float64) >= t)), t

    def cut(self, t):
        """int32 (N,): the clusters at kinship >= t, each proband labelled with the smallest position in its cluster (the `label` of
        gen.phiClusters at threshold t).  ValueError for t < floor or NaN."""
        k, _ = self._passing(t)
        parent = list(range(self.n))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for a, b in zip(self.row[:k].tolist(), self.col[:k].tolist()):
            a, b = find(a), find(b)
            parent[max(a, b)] = min(a, b)                       # the root of a cluster is its smallest position
        return np.array([find(i) for i in range(self.n)], dtype=np.int32)

    def clusters(self, t):
        """The PhiClusters of gen.phiClusters at threshold t (its `n_pairs` is None: the tree never counts the pairs)."""
        label = self.cut(t)
        return PhiClusters(_threshold(t), self.pro, label, None)

    def heights(self):
        """(kinship float32 (H,), n_clusters int64 (H,)): the distinct kinships at which something merges, descending, and the
        number of clusters left once every merge at or above each has happened."""
        if not len(self.kinship):
            return np.empty(0, dtype=np.float32), np.empty(0, dtype=np.int64)
        last = np.flatnonzero(np.append(self.kinship[1:] != self.kinship[:-1], True))       # the last edge of every run of equals
        return self.kinship[last].copy(), (self.n - (last + 1)).astype(np.int64)

    def linkage(self):
        """float64 (N - 1, 4): the merge table in SciPy's convention (scipy.cluster.hierarchy; SciPy itself is not needed): row k
        holds the two clusters that edge k joins, the smaller id first, the distance 1 - kinship, and the size of the new cluster,
        which gets the id N + k; the ids 0 .. N - 1 are the probands.  ValueError unless the tree is one piece (n_trees == 1)."""
        if self.n_trees != 1:
            raise ValueError("PhiTree.linkage: %d trees at kinship >= %g: a merge table needs one (build the tree with a lower floor)" % (
                self.n_trees, self.floor))
        n = self.n
        parent, ident, size = list(range(n)), list(range(n)), [1] * n
        out = np.empty((len(self.row), 4), dtype=np.float64)

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for k, (a, b, phi) in enumerate(zip(self.row.tolist(), self.col.tolist(), self.kinship.astype(np.float64).tolist())):
            a, b = find(a), find(b)
            out[k] = (min(ident[a], ident[b]), max(ident[a], ident[b]), 1.0 - phi, size[a] + size[b])
            parent[b] = a
            ident[a], size[a] = n + k, size[a] + size[b]
        return out


def phiTree(x, floor=None, probandIDs=None, device=None):
    """The single-linkage tree of the kinships: which probands merge at which kinship, from the closest pairs down to `floor` -- the
    families of gen.phiClusters at every cutoff at once.  Returns a PhiTree.  Neither GENLIB nor the reference has this function.

    The edges are the pairs i < j with float64(Phi[i, j]) >= floor (gen.phiOver's rule); floor None is the smallest positive
    Float32, "any positive kinship"; floor <= 0 makes every pair an edge.  Edge (i, j) precedes (i', j') when its kinship is larger,
    then when i is smaller, then when j is smaller; an edge belongs to the tree iff no path of preceding edges joins its ends
    (Kruskal's rule), so the answer is unique.  PhiTree.cut(t) gives gen.phiClusters' labels at any t >= floor.

    x a Pedigree: gen.phi's sweep for probandIDs (default gen.pro; duplicates collapse, as gen.phi does), then Boruvka's rounds on the
    device over the rows of the resident matrix, which is never copied and whose pairs are never listed or sorted
    (genphi_result_tree).  x a square host matrix: Kruskal's loop over the sorted upper triangle in numpy, rounds = 0.
    ValueError for a NaN floor, KeyError for an unknown proband ID."""
    floor = _capi.tree_floor(floor)
    if floor != floor:
        raise ValueError("the floor is NaN")
    if isinstance(x, Pedigree):
        ids, (row, col, kinship, n_trees, rounds) = _resident_query(x, probandIDs, device, lambda pl: pl.tree(floor))
        return PhiTree(floor, ids, len(ids), row, col, kinship, n_trees, rounds)
    m = np.asarray(x, dtype=np.float32)
    _, ids = _host_matrix(m, probandIDs, "gen.phiTree")
    n = len(m)
    i, j = np.triu_indices(n, 1)
    phi = m[i, j]
    keep = phi.astype(np.float64) >= floor
    i, j, phi = i[keep], j[keep], phi[keep]
    order = np.lexsort((j, i, -phi.astype(np.float64)))         # larger kinship, then smaller row, then smaller column
    i, j = i[order], j[order]
    parent = np.arange(n)
    taken = []
    for lo in range(0, len(order), 1 << 15):                    # in slices: the edges inside a cluster drop out in numpy
        if len(taken) == n - 1:
            break
        while True:                                             # parent -> the root of every position
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
        a, b = i[lo:lo + (1 << 15)], j[lo:lo + (1 << 15)]
        live = np.flatnonzero(parent[a] != parent[b])
        for e in live.tolist():
            ra, rb = int(a[e]), int(b[e])
            while parent[ra] != ra:
                ra = int(parent[ra])
            while parent[rb] != rb:
                rb = int(parent[rb])
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
                taken.append(lo + e)
    taken = np.asarray(taken, dtype=np.int64)
    row, col = i[taken].astype(np.int32), j[taken].astype(np.int32)
    return PhiTree(floor, ids, n, row, col, m[row, col], n - len(taken), 0)


class PhiNearest:
    """What gen.phiNearest returns: for each of the N probands its `k` closest relatives, closest first.  `pro` (int64, the N IDs in
    the order of the rows, None when no IDs were given with a host matrix), `index` (int32 (N, k), 0-based positions in that order),
    `relative` (int64 (N, k), the IDs at those positions, None without `pro`) and `kinship` (float32 (N, k), the matrix entries bit
    for bit)."""

    def __init__(self, k, pro, index, relative, kinship):
        self.k, self.pro, self.index, self.relative, self.kinship = k, pro, index, relative, kinship

    def __len__(self):
        return len(self.index)

    def __repr__(self):
        lines = ["PhiNearest: the %d nearest relatives of %d probands" % (self.k, len(self))]
        for r in range(min(len(self), 5)):
            who = r if self.pro is None else self.pro[r]
            rel = self.index[r] if self.relative is None else self.relative[r]
            lines.append("%d: %s" % (who, " ".join("%d (%.6g)" % (a, b) for a, b in zip(rel[:3], self.kinship[r, :3]))) +
                         (" ..." if self.k > 3 else ""))
        if len(self) > 5:
            lines.append("...")
        return "\n".join(lines)


def phiNearest(x, k=10, probandIDs=None, device=None):
    """Each proband's k closest relatives.  Returns a PhiNearest.  Neither GENLIB nor the reference has this function.

    x a Pedigree: gen.phi's sweep for probandIDs (default gen.pro), then the selection on the device from the resident matrix,
    which is never copied (genphi_result_nearest; one pass over its rows).  x a square host matrix: the same selection
    in numpy; `pro` and `relative` come from probandIDs if given.

    The candidates of proband i are the probands j != i, ordered by larger Phi[i, j] first and smaller position j first among
    equal values; positions are 0-based in the order of the probands (duplicate probandIDs collapsed, as gen.phi does).  k is
    clipped to N - 1.  ValueError for k < 1, for k > 64 after clipping, or for fewer than 2 probands; KeyError for an unknown
    proband ID."""
    k = int(k)
    if k < 1:
        raise ValueError("gen.phiNearest: k = %d, need k >= 1" % k)

    def clipped(n):
        if n < 2:
            raise ValueError("gen.phiNearest: %d proband%s: nobody has a nearest relative" % (n, "" if n == 1 else "s"))
        if min(k, n - 1) > _capi.GENPHI_NEAREST_MAX_K:
            raise ValueError("gen.phiNearest: k = %d, at most %d" % (min(k, n - 1), _capi.GENPHI_NEAREST_MAX_K))
        return min(k, n - 1)

    if isinstance(x, Pedigree):
        ids = pro(x) if probandIDs is None else np.ascontiguousarray(probandIDs, dtype=np.int64)
        x.positions(ids)                                        # KeyError on an unknown ID
        _, first = np.unique(ids, return_index=True)
        uniq = ids[np.sort(first)]                              # duplicates collapse: first occurrences, in order
        kk = clipped(len(uniq))
        pl, key = _plan_for(x, ids, device)
        keep = False
        try:
            pl.compute_device(device=device)
            index, kinship = pl.nearest(kk)
            keep = key is not None and _keep_plan(x, key, pl, ids)
        finally:
            if not keep:
                if key is not None and key in x._plans and x._plans[key][0] is pl:
                    del x._plans[key]
                pl.close()
        return PhiNearest(kk, uniq, index, uniq[index], kinship)
    m = np.asarray(x, dtype=np.float32)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError("gen.phiNearest takes a Pedigree or a square kinship matrix, got shape %s" % (m.shape,))
    ids = None if probandIDs is None else np.asarray(probandIDs, dtype=np.int64)
    if ids is not None and ids.shape != (len(m),):
        raise ValueError("probandIDs must name the %d rows of the matrix" % len(m))
    kk = clipped(len(m))
    neg = -m.astype(np.float64)
    np.fill_diagonal(neg, np.inf)                               # the diagonal comes last: never among the N - 1 candidates
    index = np.argsort(neg, axis=1, kind="stable")[:, :kk].astype(np.int32)     # stable: equal values by smaller column
    return PhiNearest(kk, ids, index, None if ids is None else ids[index], np.take_along_axis(m, index, axis=1))


def _resident_query(x, probandIDs, device, query):
    """(the probands, each once, in order; query(plan)) after gen.phi's sweep of pedigree x through the plan cache."""
    ids = pro(x) if probandIDs is None else np.ascontiguousarray(probandIDs, dtype=np.int64)
    x.positions(ids)                                            # KeyError on an unknown ID
    _, first = np.unique(ids, return_index=True)
    uniq = ids[np.sort(first)]                                  # duplicates collapse: first occurrences, in order
    pl, key = _plan_for(x, ids, device)
    keep = False
    try:
        pl.compute_device(device=device)
        out = query(pl)
        keep = key is not None and _keep_plan(x, key, pl, ids)
    finally:
        if not keep:
            if key is not None and key in x._plans and x._plans[key][0] is pl:
                del x._plans[key]
            pl.close()
    return uniq, out


def _host_matrix(x, probandIDs, who):
    """(float64 square matrix from a host Float32 kinship matrix, its IDs or None)."""
    m = np.asarray(x, dtype=np.float32)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError("%s takes a Pedigree or a square kinship matrix, got shape %s" % (who, m.shape))
    ids = None if probandIDs is None else np.asarray(probandIDs, dtype=np.int64)
    if ids is not None and ids.shape != (len(m),):
        raise ValueError("probandIDs must name the %d rows of the matrix" % len(m))
    return m.astype(np.float64), ids


def phiMatmul(x, X, probandIDs=None, device=None):
    """The product Phi @ X of the kinship matrix with a vector or a tall, skinny matrix X (one row per proband), float64.  Neither
    GENLIB nor the reference has this function: it is the primitive under quadratic forms, projections and iterative solvers.

    x a Pedigree: gen.phi's sweep for probandIDs (default gen.pro; duplicates collapse, as gen.phi does), then the product on the
    device from the resident matrix, which is never copied (genphi_result_matmul).  x a square host matrix: the same
    product in numpy Float64 (another order of the additions).  A 1-D X gives a 1-D result.  ValueError for a wrong shape, KeyError
    for an unknown proband ID."""
    if isinstance(x, Pedigree):
        return _resident_query(x, probandIDs, device, lambda pl: pl.matmul(X))[1]
    m, _ = _host_matrix(x, probandIDs, "gen.phiMatmul")
    X, one = _capi.as_panel(X, len(m), "X")
    out = m @ X
    return out[:, 0] if one else out


class PhiHist:
    """What gen.phiHist returns: `edges` (float64, bins + 1 of them), `counts` (int64: one per bin, or (groups, groups, bins) and
    symmetric with `groups`), `below` / `above` (the pairs left of the first and right of the last edge: ints, or (groups, groups)),
    `n_pairs` (the pairs counted) and, with `groups`, `names` (sorted) and `sizes` (probands per group); both None without."""

    def __init__(self, edges, counts, below, above, n_pairs, names=None, sizes=None):
        self.edges, self.counts, self.below, self.above, self.n_pairs, self.names, self.sizes = edges, counts, below, above, n_pairs, names, sizes

    def __repr__(self):
        bins = len(self.edges) - 1
        head = "PhiHist: %d pairs in %d bins over [%g, %g]" % (self.n_pairs, bins, self.edges[0], self.edges[-1])
        if self.names is None:
            total = self.counts
            lines = [head + ", %d below, %d above" % (self.below, self.above)]
        else:
            upper = np.triu(np.ones(self.below.shape, dtype=bool))
            total = self.counts[upper].sum(axis=0)
            lines = [head + ", %d groups (%s)" % (len(self.names), ", ".join("%s n=%d" % (n, s) for n, s in zip(self.names, self.sizes)))]
        for b in np.argsort(-total, kind="stable")[:5]:
            if total[b]:
                lines.append("[%g, %g%s %d" % (self.edges[b], self.edges[b + 1], "]" if b == bins - 1 else ")", total[b]))
        return "\n".join(lines)


def _hist_numpy(m, edges, labels=None, n_groups=None):
    """genphi_result_hist's definition (include/genphi.h) on a square host matrix, in numpy: (counts, below, above)."""
    n, bins = len(m), len(edges) - 1
    i, j = np.triu_indices(n, 1)
    x = m[i, j].astype(np.float64)
    k = np.searchsorted(edges, x, side="right")                 # 0: below; n_edges: at or above the last edge
    k = np.where((k == bins + 1) & (x == edges[-1]), bins, k)   # the last bin is closed
    if labels is None:
        t = np.bincount(k, minlength=bins + 2).astype(np.int64)
        return t[1:bins + 1], int(t[0]), int(t[bins + 1])
    g = int(n_groups)
    a, b = labels[i].astype(np.int64), labels[j].astype(np.int64)
    keep = (a >= 0) & (b >= 0)
    a, b, k = a[keep], b[keep], k[keep]
    t = np.bincount((a * g + b) * (bins + 2) + k, minlength=g * g * (bins + 2)).astype(np.int64).reshape(g, g, bins + 2)
    t = t + np.transpose(t, (1, 0, 2)) * (1 - np.eye(g, dtype=np.int64))[:, :, None]
    return np.ascontiguousarray(t[:, :, 1:bins + 1]), np.ascontiguousarray(t[:, :, 0]), np.ascontiguousarray(t[:, :, bins + 1])


def _hist_edges(bins, span):
    if np.ndim(bins) == 0:
        nb = int(bins)
        lo, hi = float(span[0]), float(span[1])
        if nb < 1 or not lo < hi:
            raise ValueError("gen.phiHist: bins = %d over the range (%r, %r)" % (nb, lo, hi))
        edges = np.linspace(lo, hi, nb + 1, dtype=np.float64)
    else:
        edges = np.ascontiguousarray(bins, dtype=np.float64)
    if edges.ndim != 1 or not 2 <= len(edges) <= _capi.GENPHI_HIST_MAX_EDGES:
        raise ValueError("gen.phiHist: %d edges, need 2 .. %d" % (edges.size, _capi.GENPHI_HIST_MAX_EDGES))
    if np.isnan(edges).any() or not np.all(edges[:-1] < edges[1:]):
        raise ValueError("gen.phiHist: the edges must be strictly increasing and not NaN")
    return edges


def phiHist(x, bins=64, range=(0.0, 0.5), groups=None, probandIDs=None, device=None):
    """The distribution of the pairwise kinships: the histogram of Phi[i, j] over all pairs i < j of probands, and with `groups`
    within and between sub-populations.  Returns a PhiHist.  Neither GENLIB nor the reference has this function.

    bins: a number of uniform bins over `range` (edges = np.linspace(lo, hi, bins + 1), float64), or the edges themselves; bins are
    numpy.histogram's (edges[b] <= x < edges[b + 1], the last one closed), and the pairs outside the edges are counted in `below` and
    `above`.  groups: a mapping ID -> group name, as gen._pop returns; probandIDs default to its keys, IDs that are not in it take
    part in no count (as in gen.phiMeanGroups); counts[a, b] counts the pairs with one member in names[a] and the other in
    names[b].

    x a Pedigree: gen.phi's sweep for the probands (default gen.pro; duplicates collapse), then the counting on the device from the
    resident matrix, which is never copied (genphi_result_hist; one read of its upper triangle).  x a square host
    matrix: the same definition in numpy; with `groups`, probandIDs must name its rows.  ValueError for edges that are not strictly
    increasing, more than 4,096 bins, more than 256 groups or more than 16,384 groups x bins; KeyError for an unknown proband ID."""
    edges = _hist_edges(bins, range)
    if isinstance(x, Pedigree):
        if groups is None:
            _, (counts, below, above) = _resident_query(x, probandIDs, device, lambda pl: pl.hist(edges))
            return PhiHist(edges, counts, below, above, int(counts.sum()) + below + above)
        names, ids, labels = _group_order(groups, probandIDs)
        _, (counts, below, above) = _resident_query(x, ids, device, lambda pl: pl.hist(edges, labels, len(names)))
    else:
        m, ids = _host_matrix(x, probandIDs, "gen.phiHist")
        if groups is None:
            counts, below, above = _hist_numpy(m, edges)
            return PhiHist(edges, counts, below, above, int(counts.sum()) + below + above)
        if len(groups) == 0:
            raise ValueError("groups is empty")
        if ids is None:
            raise ValueError("gen.phiHist: groups of a host matrix need probandIDs, the IDs of its rows")
        names = sorted(set(groups.values()))
        index = {name: k for k, name in enumerate(names)}
        labels = np.array([index[groups[i]] if i in groups else -1 for i in ids.tolist()], dtype=np.int32)
        if len(names) > _capi.GENPHI_HIST_MAX_GROUPS or len(names) * (len(edges) - 1) > _capi.GENPHI_HIST_MAX_CELLS:
            raise ValueError("gen.phiHist: %d groups x %d bins: at most %d groups and %d cells" % (
                len(names), len(edges) - 1, _capi.GENPHI_HIST_MAX_GROUPS, _capi.GENPHI_HIST_MAX_CELLS))
        counts, below, above = _hist_numpy(m, edges, labels, len(names))
    upper = np.triu(np.ones(below.shape, dtype=bool))
    sizes = np.bincount(labels[labels >= 0], minlength=len(names)).astype(np.int64)
    return PhiHist(edges, counts, below, above, int(counts[upper].sum() + below[upper].sum() + above[upper].sum()), names, sizes)


def phiQuantile(x, q, probandIDs=None, device=None):
    """Quantiles of the pairwise kinships Phi[i, j], i < j: a float64 array with one entry per q in [0, 1] (q = 0.5: the median).
    Neither GENLIB nor the reference has this function; a gen.phiOver threshold is chosen from it.

    With n pairs sorted ascending and h = q (n - 1): lo + (hi - lo) (h - floor(h)) in float64, lo and hi being the entries of rank
    floor(h) and ceil(h) -- numpy.quantile's "linear" method on the exact order statistics.

    x a Pedigree: gen.phi's sweep for probandIDs (default gen.pro; duplicates collapse), then a radix selection on the device from
    the resident matrix, which is never copied (genphi_result_select; 8 quantiles per device call, each call four
    reads of the upper triangle).  x a square host matrix: the same definition by a numpy sort.  ValueError for a q outside [0, 1]
    or fewer than 2 probands; KeyError for an unknown proband ID."""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if q.ndim != 1 or np.isnan(q).any() or np.any(q < 0) or np.any(q > 1):
        raise ValueError("gen.phiQuantile: q must be numbers in [0, 1]")

    def ranks_of(n):
        if n < 1:
            raise ValueError("gen.phiQuantile: no pair of probands")
        h = q * (n - 1)
        lo = np.floor(h)
        return h - lo, lo.astype(np.int64), np.ceil(h).astype(np.int64)

    if isinstance(x, Pedigree):
        def query(pl):
            frac, lo, hi = ranks_of(pl.count_pairs())
            v_lo, v_hi = np.empty(len(q), dtype=np.float64), np.empty(len(q), dtype=np.float64)
            for k in np.arange(0, len(q), _capi.GENPHI_SELECT_MAX_RANKS // 2):               # 8 quantiles = 16 ranks per call
                part = slice(k, k + _capi.GENPHI_SELECT_MAX_RANKS // 2)
                got = pl.select(np.concatenate([lo[part], hi[part]])).astype(np.float64)
                v_lo[part], v_hi[part] = got[:len(lo[part])], got[len(lo[part]):]
            return frac, v_lo, v_hi
        _, (frac, v_lo, v_hi) = _resident_query(x, probandIDs, device, query)
    else:
        m, _ = _host_matrix(x, probandIDs, "gen.phiQuantile")
        s = np.sort(m[np.triu_indices(len(m), 1)])
        frac, lo, hi = ranks_of(len(s))
        v_lo, v_hi = s[lo], s[hi]
    return v_lo + (v_hi - v_lo) * frac


class PhiEigen:
    """What gen.phiEigen returns: `values` (float64 (k,), descending), `vectors` (float64 (N, k): unit columns, the component of largest
    magnitude positive), `residual` (float64 (k,): the true ||Op v - theta v||_2), `converged` (bool (k,)), `products` (the Lanczos steps
    taken; 0 by numpy.linalg.eigh), `pro` (int64, the N IDs in the order of the rows; None when no IDs were given with a host matrix),
    `center`, `tol`, and `coordinates` = vectors * sqrt(max(values, 0)): with center=True the principal coordinates."""

    def __init__(self, values, vectors, residual, converged, products, pro, center, tol):
        self.values, self.vectors, self.residual, self.converged, self.products = values, vectors, residual, converged, products
        self.pro, self.center, self.tol = pro, center, tol

    @property
    def coordinates(self):
        return self.vectors * np.sqrt(np.maximum(self.values, 0.0))

    def __len__(self):
        return len(self.vectors)

    def __repr__(self):
        k = len(self.values)
        return "PhiEigen: %d largest eigenpair%s of %s for %d probands; %d converged to tol = %g in %d products; values %s; largest residual %.3g" % (
            k, "" if k == 1 else "s", "J Phi J" if self.center else "Phi", len(self), int(np.count_nonzero(self.converged)), self.tol, self.products,
            " ".join("%.6g" % v for v in self.values[:4]) + (" .." if k > 4 else ""), float(np.max(self.residual)) if k else 0.0)


def _eigen_sign(v):
    """Each column with its component of largest magnitude (the first among equals) made positive."""
    big = np.argmax(np.abs(v), axis=0)
    s = np.where(v[big, np.arange(v.shape[1])] < 0.0, -1.0, 1.0)
    return v * s


def phiEigen(x, k=10, center=False, tol=1e-8, maxiter=300, seed=0, probandIDs=None, device=None):
    """The k algebraically largest eigenpairs of the kinship matrix Phi: the top of its spectrum and, with center=True (Gower's
    centring J Phi J, J = I - 11^T / N), the principal coordinates of population structure.  Returns a PhiEigen.  Neither GENLIB nor
    the reference has this function; include/genphi.h is its definition.

    x a Pedigree: gen.phi's sweep for probandIDs (default gen.pro; duplicates collapse), then Lanczos with full reorthogonalisation on
    the device with the resident matrix, which is never copied (genphi_result_eigen): the Krylov basis and the Ritz vectors
    stay on the device, a start vector drawn from `seed`, stopped when the k pairs satisfy beta |s| <= tol theta_1 or after
    min(maxiter, N) products.  `converged` and the true `residual` say how far each pair got.  x a square host matrix: the same
    definition by numpy.linalg.eigh on the Float64 matrix (products = 0).

    One Krylov sequence finds one vector per distinct eigenvalue: an eigenvalue that is repeated among the top k is reported ONCE and
    the list goes on with the next distinct ones (eigh lists every copy); further copies appear only after a breakdown (unrelated
    founders, Phi = I / 2) or when the iteration runs on far beyond convergence.

    ValueError for k outside [1, min(64, N)], a negative or NaN tol, maxiter outside [k, 4096]; KeyError for an unknown proband ID."""
    k, tol, maxiter, center = int(k), float(tol), int(maxiter), bool(center)
    if not tol >= 0.0:
        raise ValueError("gen.phiEigen: tol = %r is negative or NaN" % tol)
    if not 1 <= k <= _capi.GENPHI_EIGEN_MAX_K:
        raise ValueError("gen.phiEigen: k = %d outside [1, %d]" % (k, _capi.GENPHI_EIGEN_MAX_K))
    if not k <= maxiter <= _capi.GENPHI_EIGEN_MAX_ITER:
        raise ValueError("gen.phiEigen: maxiter = %d outside [k = %d, %d]" % (maxiter, k, _capi.GENPHI_EIGEN_MAX_ITER))
    if isinstance(x, Pedigree):
        ids, (val, vec, res, conv, prod) = _resident_query(x, probandIDs, device, lambda pl: pl.eigen(k, center, tol, maxiter, seed))
        return PhiEigen(val, vec, res, conv, prod, ids, center, tol)
    m, ids = _host_matrix(x, probandIDs, "gen.phiEigen")
    n = len(m)
    if k > n:
        raise ValueError("gen.phiEigen: k = %d outside [1, N = %d]" % (k, n))
    if center:
        m = m - m.mean(axis=0)[None, :]
        m = m - m.mean(axis=1)[:, None]
        m = (m + m.T) / 2
    lam, vec = np.linalg.eigh(m)
    val, vec = lam[::-1][:k].copy(), _eigen_sign(np.ascontiguousarray(vec[:, ::-1][:, :k]))
    res = np.sqrt(((m @ vec - vec * val) ** 2).sum(axis=0))
    return PhiEigen(val, vec, res, res <= tol * val[0] + (n + 2) * 2.0 ** -53 * abs(val[0]), 0, ids, center, tol)


class PhiSolve:
    """What gen.phiSolve returns: `solution` (float64, the shape of B), per right-hand side `residual` (float64, the true relative
    residual ||b - (Phi + ridge I) z|| / ||b||), `iterations` (int32, products of the iteration) and `converged` (residual <= tol);
    `pro` (int64, the N IDs in the order of the rows, None when no IDs were given with a host matrix), `ridge` and `tol`."""

    def __init__(self, solution, residual, iterations, tol, ridge, pro):
        self.solution, self.residual, self.iterations, self.tol, self.ridge, self.pro = solution, residual, iterations, tol, ridge, pro
        self.converged = residual <= tol

    def __len__(self):
        return len(self.solution)

    def __repr__(self):
        k = len(self.residual)
        return "PhiSolve: (Phi + %g I) z = b for %d probands, %d right-hand side%s; %d converged to tol = %g; iterations %s, largest residual %.3g" % (
            self.ridge, len(self), k, "" if k == 1 else "s", int(np.count_nonzero(self.converged)), self.tol,
            "-" if k == 0 else "%d .. %d" % (self.iterations.min(), self.iterations.max()), self.residual.max() if k else 0.0)


def _cg_numpy(a, b, ridge, tol, maxiter):
    """genphi_result_solve's iteration (include/genphi.h) in numpy Float64 on a host matrix: (z, residual, iterations)."""
    n, k = b.shape
    z, res, its = np.zeros((n, k)), np.zeros(k), np.zeros(k, dtype=np.int32)
    for c in range(k):
        bc = b[:, c]
        nb = np.sqrt(bc @ bc)
        if nb == 0.0:
            continue
        zc, r, d = np.zeros(n), bc.copy(), bc.copy()
        rho = r @ r
        if not nb <= tol * nb:
            for _ in range(maxiter):
                q = a @ d + ridge * d
                its[c] += 1
                g = d @ q
                if not g > 0.0 or not np.isfinite(g):
                    break
                alpha = rho / g
                zc += alpha * d
                r -= alpha * q
                rho_new = r @ r
                if np.sqrt(rho_new) <= tol * nb:
                    break
                d = r + (rho_new / rho) * d
                rho = rho_new
        z[:, c] = zc
        e = bc - (a @ zc + ridge * zc)
        res[c] = np.sqrt(e @ e) / nb
    return z, res, its


def phiSolve(x, B, ridge=0.0, tol=1e-10, maxiter=1000, probandIDs=None, device=None):
    """Solves (Phi + ridge I) z = B, the system under the animal model, BLUP and heritability: (2 Phi s2g + I s2e)^-1 y with
    ridge = s2e / (2 s2g).  Returns a PhiSolve.  Neither GENLIB nor the reference has this function.

    x a Pedigree: gen.phi's sweep for probandIDs (default gen.pro; duplicates collapse), then conjugate gradients over the product
    on the device with the resident matrix, which is never copied (genphi_result_solve): textbook CG from z = 0, every
    column with its own scalars, stopped when the recurrence residual is <= tol ||b||, when the curvature d.Ad is not positive or not
    finite, or after maxiter products; the residual reported is the true one, from one more product.  x a square host matrix: the
    same iteration in numpy Float64.  B is (N,) or (N, k).  ValueError for a wrong shape, a negative or non-finite ridge, a negative
    or NaN tol, maxiter < 1; KeyError for an unknown proband ID."""
    ridge, tol, maxiter = float(ridge), float(tol), int(maxiter)
    if not ridge >= 0.0 or not np.isfinite(ridge):
        raise ValueError("gen.phiSolve: ridge = %r is negative or not finite" % ridge)
    if not tol >= 0.0:
        raise ValueError("gen.phiSolve: tol = %r is negative or NaN" % tol)
    if not 1 <= maxiter < 2 ** 31:
        raise ValueError("gen.phiSolve: maxiter = %d, need at least 1" % maxiter)
    if isinstance(x, Pedigree):
        ids, (z, res, its) = _resident_query(x, probandIDs, device, lambda pl: pl.solve(B, ridge, tol, maxiter))
        return PhiSolve(z, res, its, tol, ridge, ids)
    m, ids = _host_matrix(x, probandIDs, "gen.phiSolve")
    B, one = _capi.as_panel(B, len(m), "B")
    z, res, its = _cg_numpy(m, B, ridge, tol, maxiter)
    return PhiSolve(z[:, 0] if one else z, res, its, tol, ridge, ids)


DEFAULT_CI_PROB = (0.025, 0.05, 0.95, 0.975)


class PhiCI:
    """What gen.phiCI and gen.fCI return: `prob` and the `quantiles` of the bootstrap distribution at them (float64, linear
    interpolation of the sorted values: R's type 7), `mean` (the observed statistic: gen.phiMean of the matrix, or the mean of
    vectF), `thetastar` (float64, the statistic of each of the `b` resamples, in resample order) and the `seed` that repeats them."""

    def __init__(self, prob, quantiles, mean, thetastar, b, seed):
        self.prob, self.quantiles, self.mean, self.thetastar, self.b, self.seed = prob, quantiles, mean, thetastar, b, seed

    def __repr__(self):
        return "PhiCI: mean %.6g, b = %d\n" % (self.mean, self.b) + "\n".join("%g%% %.6g" % (100 * p, q) for p, q in zip(self.prob, self.quantiles))


def _ci_args(prob, b, seed):
    prob = np.atleast_1d(np.asarray(prob, dtype=np.float64))
    if prob.ndim != 1 or not np.all((prob >= 0) & (prob <= 1)):            # (a NaN fails both comparisons)
        raise ValueError("prob must lie in [0, 1]")
    b = int(b)
    if not 1 <= b < 2 ** 31:
        raise ValueError("b = %d resamples: need 1 <= b < 2^31" % b)
    if seed is None:
        import secrets
        seed = secrets.randbits(64)
    return prob, b, int(seed) & 0xFFFFFFFFFFFFFFFF


_CI_HOST_BLOCK = 256          # resamples per block of the host routes (a block of counts is n x 256 float64)


def phiCI(x, prob=DEFAULT_CI_PROB, b=5000, seed=None, probandIDs=None, device=None):
    """GENLIB's gen.phiCI(phiMatrix, prob, b = 5000): the bootstrap confidence interval of the mean kinship.  Returns a PhiCI.

    A resample draws the N probands N times with replacement and takes gen.phiMean of the resampled matrix Phi[s, s]; with c[i]
    the number of times proband i was drawn that is (c' Phi c - sum_i c[i] Phi[i, i]) / (N (N - 1)) (a proband drawn twice puts its
    self-kinship at two off-diagonal positions, which stay in).  The draws are Philox4x32-10 keyed on (seed, resample, draw): a
    pure function of (N, seed, resample), the same on the host and on the device (include/genphi.h).  seed=None draws 64 fresh
    bits (secrets.randbits); .seed reports them.

    x a Pedigree: gen.phi's sweep for probandIDs (default gen.pro), then genphi_result_bootstrap on the resident matrix, which is
    never copied: a Float64 product of the matrix with the counts of a panel of resamples, fused with its reduction.
    x a square host matrix (GENLIB's own signature): the same counts (genphi_bootstrap_counts) and numpy in Float64.

    GENLIB's 3-D input (kinship by depth) and print.it are not offered.  ValueError for fewer than 2 probands, b < 1, a prob
    outside [0, 1] or a matrix that is not square; KeyError for an unknown proband ID."""
    prob, b, seed = _ci_args(prob, b, seed)
    if isinstance(x, Pedigree):
        ids = pro(x) if probandIDs is None else np.ascontiguousarray(probandIDs, dtype=np.int64)
        x.positions(ids)                                        # KeyError on an unknown ID
        n = len(np.unique(ids))
        if n < 2:
            raise ValueError("gen.phiCI needs at least 2 probands, got %d" % n)
        pl, key = _plan_for(x, ids, device)
        keep = False
        try:
            pl.compute_device(device=device)
            total, diagonal, _ = pl.result_sums()
            quad, own = pl.bootstrap(b, seed)
            keep = key is not None and _keep_plan(x, key, pl, ids)
        finally:
            if not keep:
                if key is not None and key in x._plans and x._plans[key][0] is pl:
                    del x._plans[key]
                pl.close()
        mean = np.float32((total - diagonal) / (n * n - n))
    else:
        m = np.asarray(x)
        if m.ndim != 2 or m.shape[0] != m.shape[1]:
            raise ValueError("gen.phiCI takes a Pedigree or a square kinship matrix, got shape %s" % (m.shape,))
        n = len(m)
        if n < 2:
            raise ValueError("gen.phiCI needs at least 2 probands, got %d" % n)
        mean = phiMean(m)
        m = m.astype(np.float64)
        diag = np.ascontiguousarray(np.diagonal(m))
        quad, own = np.empty(b, dtype=np.float64), np.empty(b, dtype=np.float64)
        for first in range(0, b, _CI_HOST_BLOCK):
            c = _capi.bootstrap_counts(n, seed, min(_CI_HOST_BLOCK, b - first), first).astype(np.float64)     # (resamples, n)
            quad[first:first + len(c)] = np.einsum("ri,ri->r", c @ m, c)
            own[first:first + len(c)] = c @ diag
    theta = (quad - own) / (float(n) * (n - 1))
    return PhiCI(prob, np.quantile(theta, prob), mean, theta, b, seed)


def fCI(vectF, prob=DEFAULT_CI_PROB, b=5000, seed=None):
    """GENLIB's gen.fCI(vectF, prob, b = 5000): the bootstrap confidence interval of the mean inbreeding.  vectF holds one inbreeding
    coefficient per proband (gen.f); a resample draws the N probands N times with replacement, with gen.phiCI's draws, and takes
    the mean sum_i c[i] F[i] / N.  On the host, in Float64.  Returns a PhiCI whose `mean` is the mean of vectF.
    ValueError for fewer than 2 values, b < 1 or a prob outside [0, 1]."""
    prob, b, seed = _ci_args(prob, b, seed)
    F = np.asarray(vectF, dtype=np.float64)
    if F.ndim != 1 or len(F) < 2:
        raise ValueError("gen.fCI takes a vector of at least 2 inbreeding coefficients, got shape %s" % (F.shape,))
    n = len(F)
    theta = np.empty(b, dtype=np.float64)
    for first in range(0, b, _CI_HOST_BLOCK):
        c = _capi.bootstrap_counts(n, seed, min(_CI_HOST_BLOCK, b - first), first).astype(np.float64)
        theta[first:first + len(c)] = (c @ F) / n
    return PhiCI(prob, np.quantile(theta, prob), float(F.sum() / n), theta, b, seed)
