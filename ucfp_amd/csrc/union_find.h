// union_find.h -- lock-free union-find over a u32 parent array in global memory (device functions).
//
// Invariants: parent[x] <= x, and parent[x] lies in x's component.  A root (parent[x] == x) only ever changes by
// one compare-and-swap that hooks it under a SMALLER root, so the root of a finished component is its smallest
// element.  Parents only decrease, so a stale read costs iterations, never correctness.  The XCDs' L2s are not
// coherent inside a launch: every access to `parent` is a relaxed agent-scope atomic, never a plain load or store.
// Used by the LSH self-join (lsh.hip); kept apart so that a later join (Hamming radius) can hook into the same forest.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ucfp {

__device__ __forceinline__ uint32_t uf_parent(const uint32_t* parent, uint32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x, halving the path on the way (a non-root never becomes a root again, and its new parent is one of its
// ancestors: racing halvings and hooks cannot break the invariants)
__device__ inline uint32_t uf_find(uint32_t* parent, uint32_t x) {
    uint32_t p = uf_parent(parent, x);
    while (p != x) {
        const uint32_t g = uf_parent(parent, p);
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

// joins the components of a and b: the larger root goes under the smaller
__device__ inline void uf_unite(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        uint32_t seen = a;
        if (__hip_atomic_compare_exchange_strong(parent + a, &seen, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        a = seen;   // another wave hooked `a` first: go on from where it points now
    }
}

}  // namespace ucfp
