"""CPU oracles for the MRCA family (gen.ancestor, gen.findFounders, gen.findMRCA, gen.findDistance, gen._findMinDistanceMRCA,
gen.meioses).  Pure Python on dictionaries; shares no code with the library.

*_literal  restate the reference line by line: ancestor() as a stack search into a set (src/identify.jl:164-199), _get_paths as
           the recursion that builds every ascending path as a list of IDs (src/describe.jl:241-259), _findDistance as the filter
           `path[0] == ancestorID` over those lists, _findMRCA as the intersection of the ancestor sets minus the ancestors of the
           intersection (src/identify.jl:97-103).  Exponential in the depth: small inputs and genea140 only.
*_exact    one breadth-first search upwards per individual (the first visit of an ancestor is its shortest ascent), the MRCA rule
           as a second search upwards from the common set.  Linear: any input.
Both must agree wherever both can run (tests/test_mrca_reference.py)."""
from collections import deque

import numpy as np


def _parents(ind, father, mother):
    return {int(i): (int(f), int(m)) for i, f, m in zip(ind, father, mother)}


# ---- literal ---------------------------------------------------------------------------------------------------------------------

def ancestor_literal(par, IDs):
    """ancestor(pedigree, ID) for an int, the sorted union for a list (src/identify.jl:164-199)."""
    if isinstance(IDs, (int, np.integer)):
        found, stack = set(), [int(IDs)]
        while stack:
            f, m = par[stack.pop()]                      # KeyError on an unknown ID, as pedigree[ID]
            if f:
                stack.append(f)
                found.add(f)
            if m:
                stack.append(m)
                found.add(m)
        return sorted(found)
    out = set()
    for i in IDs:
        out |= set(ancestor_literal(par, int(i)))
    return sorted(out)


def get_paths_literal(par, ID):
    """_get_paths: every ascending path of ID, each a list of IDs from the ancestor reached down to ID."""
    paths = [[ID]]
    f, m = par[ID]
    for p in (f, m):
        if p:
            up = get_paths_literal(par, p)
            for path in up:
                path.append(ID)
            paths.extend(up)
    return paths


def _min_distance_literal(par, ID, ancestorID, cache):
    """_findMinDistance: minimum(lengths of the paths that start at ancestorID); ValueError on an empty list as Julia's minimum."""
    if ID not in cache:                                  # (the reference enumerates again per call; the paths are the same)
        cache[ID] = get_paths_literal(par, ID)
    return min(len(path) - 1 for path in cache[ID] if path[0] == ancestorID)


def mrca_ids_literal(par, IDs):
    sets = [set(ancestor_literal(par, int(i))) for i in IDs]
    common = set.intersection(*sets)
    older = set(ancestor_literal(par, sorted(common)))
    return sorted(common - older), sorted(common)


def find_mrca_literal(ind, father, mother, IDs):
    """findMRCA: (ancestors ascending, meioses int64 (len(IDs), len(ancestors)), number of common ancestors)."""
    par = _parents(ind, father, mother)
    mrcas, common = mrca_ids_literal(par, IDs)
    cache = {}
    M = np.zeros((len(IDs), len(mrcas)), dtype=np.int64)
    for i, ID in enumerate(IDs):
        for j, a in enumerate(mrcas):
            M[i, j] = _min_distance_literal(par, int(ID), a, cache)
    return np.array(mrcas, dtype=np.int64), M, len(common)


def find_founders_literal(ind, father, mother, IDs):
    par = _parents(ind, father, mother)
    common = set.intersection(*[set(ancestor_literal(par, int(i))) for i in IDs])
    return np.array(sorted(a for a in common if par[a] == (0, 0)), dtype=np.int64)


def find_distance_literal(ind, father, mother, IDs, ancestorID):
    par = _parents(ind, father, mother)
    cache = {}
    return _min_distance_literal(par, int(IDs[0]), int(ancestorID), cache) + _min_distance_literal(par, int(IDs[1]), int(ancestorID), cache)


def min_distance_mrca_literal(ind, father, mother, IDs):
    par = _parents(ind, father, mother)
    mrcas, _ = mrca_ids_literal(par, IDs)
    cache = {}
    return min(_min_distance_literal(par, int(IDs[0]), a, cache) + _min_distance_literal(par, int(IDs[1]), a, cache) for a in mrcas)


def meioses_literal(ind, father, mother, pro, anc):
    """int16 (len(pro), len(anc)): the shortest path that starts at anc[j] among the path lists of pro[i], -1 without one."""
    par = _parents(ind, father, mother)
    for a in anc:
        par[int(a)]
    out = np.full((len(pro), len(anc)), -1, dtype=np.int16)
    for i, ID in enumerate(pro):
        best = {}
        for path in get_paths_literal(par, int(ID)):
            if path[0] not in best or len(path) - 1 < best[path[0]]:
                best[path[0]] = len(path) - 1
        for j, a in enumerate(anc):
            out[i, j] = best.get(int(a), -1)
    return out


# ---- exact -----------------------------------------------------------------------------------------------------------------------

def ascents_exact(par, ID):
    """{ancestor: meioses of the shortest ascent}, ID itself at 0: breadth-first search upwards."""
    dist = {ID: 0}
    queue = deque([ID])
    while queue:
        x = queue.popleft()
        for p in par[x]:
            if p and p not in dist:
                dist[p] = dist[x] + 1
                queue.append(p)
    return dist


def meioses_exact(ind, father, mother, pro, anc, sample=None):
    """int16 (len(pro), len(anc)), or the rows `sample` of it."""
    par = _parents(ind, father, mother)
    rows = range(len(pro)) if sample is None else [int(k) for k in sample]
    for a in anc:
        par[int(a)]
    out = np.full((len(rows), len(anc)), -1, dtype=np.int16)
    cache = {}
    for r, i in enumerate(rows):
        ID = int(pro[i])
        if ID not in cache:
            cache[ID] = ascents_exact(par, ID)
        d = cache[ID]
        out[r] = [d.get(int(a), -1) for a in anc]
    return out


def find_mrca_exact(ind, father, mother, IDs):
    """(ancestors ascending, meioses int64 (len(IDs), len(ancestors)), number of common ancestors)."""
    par = _parents(ind, father, mother)
    asc = {}
    for ID in IDs:
        if int(ID) not in asc:
            asc[int(ID)] = ascents_exact(par, int(ID))
    common = None
    for ID, d in asc.items():
        strict = set(d) - {ID}
        common = strict if common is None else common & strict
    common = common or set()
    # the ancestors of the common set: one search upwards from all of it
    older, queue = set(), deque(common)
    while queue:
        for p in par[queue.popleft()]:
            if p and p not in older:
                older.add(p)
                queue.append(p)
    mrcas = sorted(common - older)
    M = np.array([[asc[int(ID)][a] for a in mrcas] for ID in IDs], dtype=np.int64).reshape(len(IDs), len(mrcas))
    return np.array(mrcas, dtype=np.int64), M, len(common)


def find_founders_exact(ind, father, mother, IDs):
    par = _parents(ind, father, mother)
    common = None
    for ID in IDs:
        strict = set(ascents_exact(par, int(ID))) - {int(ID)}
        common = strict if common is None else common & strict
    return np.array(sorted(a for a in (common or ()) if par[a] == (0, 0)), dtype=np.int64)
