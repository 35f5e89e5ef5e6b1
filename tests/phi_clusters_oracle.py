"""The oracle of gen.phiClusters / gen.phiUnrelated (include/genphi.h: genphi_result_clusters, genphi_result_unrelated) in plain numpy
and Python loops: a boolean adjacency matrix, a breadth-first search, the literal sequential greedy loop.  It shares no trick with the
kernels: no union-find, no rounds (jacobi_rounds applies the round rule synchronously only to bound the number of launches)."""
from collections import deque

import numpy as np


def adjacency(phi, t):
    """The edges of G_t: float64(Phi[i, j]) >= t, the diagonal cleared.  phi: the square Float32 host matrix (no padding columns)."""
    phi = np.asarray(phi)
    assert phi.ndim == 2 and phi.shape[0] == phi.shape[1]
    a = phi.astype(np.float64) >= float(t)
    a = a.copy()
    np.fill_diagonal(a, False)
    return a


def components(a):
    """label int32 (N,): the smallest position of every vertex's connected component, by a breadth-first search from every vertex not
    yet reached, in ascending order."""
    n = len(a)
    label = np.full(n, -1, dtype=np.int32)
    nbrs = [np.flatnonzero(a[i]) for i in range(n)]
    for s in range(n):
        if label[s] >= 0:
            continue
        label[s] = s
        queue = deque([s])
        while queue:
            u = queue.popleft()
            fresh = nbrs[u][label[nbrs[u]] < 0]               # the neighbours reached for the first time
            label[fresh] = s
            queue.extend(fresh.tolist())
    return label


def n_pairs(a):
    return int(np.count_nonzero(np.triu(a, 1)))


def degrees(a):
    return a.sum(axis=1).astype(np.int32)


def keys(a, priority=None):
    """The visiting key of every vertex as a Python list of (priority, position) tuples; priority None: the degrees."""
    pri = degrees(a) if priority is None else np.asarray(priority)
    assert pri.shape == (len(a),)
    return [(int(pri[i]), i) for i in range(len(a))]


def greedy(a, priority=None):
    """member bool (N,): visit the vertices in ascending key order and take a vertex iff none of its neighbours has been taken."""
    n = len(a)
    key = keys(a, priority)
    member = np.zeros(n, dtype=bool)
    for i in sorted(range(n), key=lambda v: key[v]):
        if not np.any(member[a[i]]):
            member[i] = True
    return member


def jacobi_rounds(a, key):
    """The number of synchronous rounds until no vertex is undecided.  In a round every undecided vertex looks at the states of the
    round's START: it is OUT if a neighbour is IN, IN if no undecided neighbour has a smaller key, and waits otherwise.  Also returns
    the members, which must be greedy's."""
    n = len(a)
    UNDECIDED, IN, OUT = 0, 1, 2
    state = np.zeros(n, dtype=np.int8)
    order = np.empty(n, dtype=np.int64)                       # rank of every vertex in key order: smaller key <=> smaller rank
    order[sorted(range(n), key=lambda v: key[v])] = np.arange(n)
    rounds = 0
    while np.any(state == UNDECIDED):
        rounds += 1
        assert rounds <= n
        new = state.copy()
        for i in np.flatnonzero(state == UNDECIDED):
            nb = np.flatnonzero(a[i])
            if np.any(state[nb] == IN):
                new[i] = OUT
            elif not np.any((state[nb] == UNDECIDED) & (order[nb] < order[i])):
                new[i] = IN
        state = new
    return rounds, state == IN


def is_independent(a, member):
    return not np.any(a[np.ix_(member, member)])


def is_maximal(a, member):
    """Every vertex outside the set has a neighbour inside."""
    return bool(np.all(member | (a[:, member].sum(axis=1) > 0)))
