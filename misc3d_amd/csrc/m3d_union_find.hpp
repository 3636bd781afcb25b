// m3d_union_find.hpp -- the lock-free union-find the device code shares (m3d_proximity.hip, m3d_ppf_cluster.hip).
//
// parent[] invariant: parent[x] <= x, and only a root (parent[x] == x) is ever written -- by a compare-and-swap that hooks
// the LARGER of two roots under the smaller.  Pointers only decrease, so every walk ends, no cycle can form, and the root
// of a finished tree is the smallest index of its component.
//
// Coherence (MI355X: one L2 per XCD, a plain load may hit a line another XCD has since changed): the walks read parent[]
// with agent-scope atomic loads, and every write is an agent-scope compare-and-swap.  Correctness rests on the CAS return
// values alone: a stale read can only show an older -- larger or equal -- ancestor, which is still in the same tree, and a
// CAS on a "root" that has been hooked meanwhile fails and returns the new parent to continue from.  Hooking b under a
// non-root a < b is harmless for the same reason.  A flatten pass runs after the union launch has ended and may read with
// plain loads.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace m3d {

__device__ __forceinline__ uint32_t uf_load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t uf_find(const uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = uf_load(parent + x);
        if (p == x) return x;
        x = p;
    }
}
__device__ __forceinline__ void uf_unite(uint32_t* parent, uint32_t a, uint32_t b) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    for (;;) {
        if (a == b) return;
        if (a > b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        uint32_t expected = b;   // hook root b under a < b
        if (__hip_atomic_compare_exchange_strong(parent + b, &expected, a, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        b = uf_find(parent, expected);   // b was hooked meanwhile: continue from its tree's root
        a = uf_find(parent, a);
    }
}

}  // namespace m3d
