// The lock-free union-find forest over parent[0 .. n_nodes) that the kernels which join nodes share: k_cluster.hip (the links, and
// the header that argues the rule below) and k_tree.hip (the hook of a round).  parent[x] <= x at all times; x is a root when
// parent[x] == x.  Every access to parent here is an agent-scope relaxed atomic -- load, CAS or min; no plain load or store.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int kLinkThreads = 256;

__device__ inline int32_t uf_load(int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// parent[x] as the forest allows it: 0 <= parent[x] <= x.  Anything else (a caller's array that is no forest) reads as "root",
// so that a walk only ever moves to smaller, non-negative indices: never an access outside parent[0 .. x].
__device__ inline int32_t uf_parent(int32_t* parent, int32_t x) {
    const int32_t p = uf_load(parent + x);
    return (uint32_t)p <= (uint32_t)x ? p : x;
}

// The root above x (as this wave sees it), halving the path on the way: parent[x] = min(parent[x], grandparent).
__device__ inline int32_t uf_find(int32_t* parent, int32_t x) {
    int32_t p = uf_parent(parent, x);
    while (p != x) {
        const int32_t g = uf_parent(parent, p);
        if (g != p) __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

// Joins the components of a and b.  Two endpoints already under one root cost reads only (and the halving of a long path).
__device__ inline void uf_union(int32_t* parent, int32_t a, int32_t b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        const int32_t hi = max(a, b), lo = min(a, b);
        int32_t seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        if ((uint32_t)seen >= (uint32_t)hi) return;   // (no forest: see uf_parent)
        a = seen;                                     // hi got a parent meanwhile: go on from there
        b = lo;
    }
}

}  // namespace
