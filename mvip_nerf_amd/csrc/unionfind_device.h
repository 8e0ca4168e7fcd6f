// Lock-free union-find on an int32 parent array, shared by the components of a bit grid (csrc/components.hip) and the
// face components / boundary loops of a mesh (csrc/mesh_topology.hip).
//
// parent[x] is x for a root, the index of another element of x's tree otherwise (the callers keep -1 for elements that take
// no part and never pass those in).  unite(a, b) finds both roots and atomicMins the lower root into the parent of the
// higher, then goes on from what the atomic displaced until both sides meet.
//
// TERMINATION.  Every write is an atomicMin of a value below the index it is written to, onto a word that starts at its own
// index, so parent[x] <= x always: a link points to a strictly lower index, find() descends strictly and ends at a root
// after at most x steps, and no cycle can form whatever the interleaving.  Each round of unite() either ends or lowers
// max(a, b) (the displaced `old` is below the root it was read from), so it ends too.  A root is the lowest index of its
// tree and, when the launch that makes the unions has ended, of its component: the result does not depend on the order the
// unions ran in though the route does.
#pragma once
#include "common.h"

namespace mvip {
namespace unionfind {

__device__ __forceinline__ int load_parent(const int *parent, int a) {
    return __hip_atomic_load(parent + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// parent[x] <= x always, so the walk ends
__device__ __forceinline__ int find(const int *parent, int a) {
    int p = load_parent(parent, a);
    while (p != a) {
        a = p;
        p = load_parent(parent, a);
    }
    return a;
}
__device__ __forceinline__ void unite(int *parent, int a, int b) {
    for (;;) {
        a = find(parent, a);
        b = find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);            // a was a root when read; if it no longer is, parent[a] = min(old, b)
        if (old == a) return;                                //   and the tie between old and b is made next
        a = old;
    }
}

}  // namespace unionfind
}  // namespace mvip
