// union_find.h -- the lock-free union-find that the graph queries of the resident result share (clusters.hip: genphi_result_clusters;
// tree.hip: genphi_result_tree).  parent[x] <= x always; x is a root while parent[x] == x.  Every read of parent is an agent-scope
// atomic load, every write a compare-and-swap of a root (the hook) or an atomicMin with an ancestor (path halving): a word only ever
// decreases, a root that was hooked never becomes a root again, and a stale read -- the XCDs do not see each other's L2 -- costs a
// retry.  The root of a tree is its smallest node.
#pragma once
#include <hip/hip_runtime.h>

namespace genphi {

__device__ __forceinline__ int parent_of(const int *parent, int x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a node that was the root of x's tree when it was read; halves the path on the way
__device__ __forceinline__ int find_root(int *parent, int x)
{
    for (;;) {
        const int p = parent_of(parent, x);
        if (p == x) return x;
        const int g = parent_of(parent, p);
        if (g == p) return p;
        atomicMin(parent + x, g);                       // g < p: an ancestor of x, nearer the root
        x = g;
    }
}

// joins the trees of a and b; returns a node that was the root of both afterwards.  The larger root goes under the smaller.
__device__ __forceinline__ int unite(int *parent, int a, int b)
{
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return a;
        if (a < b) { const int s = a; a = b; b = s; }
        const int seen = atomicCAS(parent + a, a, b);
        if (seen == a) return b;                        // a was still a root
        a = seen;                                       // somebody hooked it first, under `seen`: go on from there (no read can stall this)
    }
}

}  // namespace genphi
