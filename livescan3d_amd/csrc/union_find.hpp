// union_find.hpp -- the lock-free union-find of the fragment filter (fragments.hip: a tick's mesh vertices joined by its triangles) and of
// background subtraction's blob pass (background.hip: kept pixels joined with their 4-neighbours, in LDS and in global memory).  Device only.
//
// parent[] is a forest over indices; a union finds an ancestor of either end and hooks the HIGHER under the LOWER, so parent[v] <= v
// holds at every moment and a tree's root is its lowest index.  How parent[] is touched:
//   - every hook is a returning atomicCAS(&parent[hi], hi, lo): it succeeds only while hi is still a root (a root is hooked once; a
//     vertex that is no root never becomes one again).  When it fails it returns what parent[hi] holds, strictly below hi, and the lane
//     goes on from there: the sum of the two indices a union holds falls with every failed round, so a union ends after at most a + b
//     rounds and no lane ever waits for another;
//   - the walks read parent[] with PLAIN loads.  Within a launch a plain load may be old (L1 is per CU, L2 per XCD), and the design is
//     correct when every one of them is: an old value of parent[x] is x itself or an earlier parent, in both cases a vertex of x's own
//     tree with an index <= x, so a walk always ends on a vertex of the right component; that it is (still) a root is decided by the CAS
//     alone, which answers with the word as it is, and hooking under a vertex that has stopped being a root still joins the two trees
//     and keeps parent[hi] < hi.  (Agent-scope atomic loads, which go past both caches, were measured in the fragment filter: the call on
//     the 8 x 512x424 scene tick took 2.7 ms with them against 2.0 ms -- fewer failed rounds do not pay for their latency.)
// A walk goes down in index with every step: at most x steps from x.  Both loops are bounded.
#pragma once

namespace {

// A vertex of x's tree that was a root when it was read.
__device__ __forceinline__ int uf_find(const int *parent, int x)
{
    int p = parent[x];
    while (p != x) {                                     // p < x: at most x rounds
        x = p;
        p = parent[x];
    }
    return x;
}

// Joins the trees of a and b; returns the root the union ended on (the lower one).
__device__ __forceinline__ int uf_unite(int *parent, int a, int b)
{
    for (;;) {                                           // a + b falls with every failed round
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return a;
        const int hi = max(a, b), lo = min(a, b);
        const int was = atomicCAS(&parent[hi], hi, lo);
        if (was == hi) return lo;
        a = was;                                         // < hi: hi had been hooked already
        b = lo;
    }
}

}  // namespace
