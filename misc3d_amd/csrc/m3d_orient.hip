// m3d_orient.hip -- the normal orientation of the PPF model preprocessing (CalcModelNormalAndSampling,
// src/ppf_estimation.cpp:1083-1148) on gfx950.  The reference's priority-queue walk is lazy Prim: what it leaves is the minimum
// spanning tree of the radius graph under the edge order (d2, lo, hi) (include/misc3d_amd.h, rules O1 - O3; DESIGN.md, "PPF
// model preprocessing"), and that tree is unique, whatever builds it.  Here it is built by Boruvka rounds over the cell-sorted
// grid; no neighbour list is materialised.
//
// Vertices are grid slots.  A round is four launches:
//   scan     one lane per slot in grid order (the lanes of a wave share rows): its least edge to a slot of another label, and
//            a 64-bit atomicMin of the bits of that d2 on the label's word (d2 >= 0 and never NaN: bit order = numeric order);
//   pick     among the slots whose own least edge has the label's d2, a 64-bit atomicMin of lo << 32 | hi -- the 128-bit key
//            (d2, lo, hi) in two passes;
//   hook     one lane per label: its edge is appended to the list and the two trees are united (m3d_union_find.hpp).  When
//            both ends' labels chose the same edge, the label that holds `hi` yields, so the edge is appended once.  Under a
//            strict total order on the edges that is the only way two labels' choices can close a cycle;
//   flatten  comp[] = the roots, the labels' words reset.
// Coherence (m3d_union_find.hpp): inside a launch every word another lane may write is touched with agent-scope atomics only
// (min_d2, min_e, parent, n_edges); everything else is read with plain loads of what an EARLIER launch wrote.
#include <hip/hip_runtime.h>

#include "m3d_orient.hpp"
#include "m3d_prox_scan.hpp"
#include "m3d_union_find.hpp"

#pragma clang fp contract(off)

namespace m3d {

namespace {

__device__ __forceinline__ void atomic_min_u64(unsigned long long* p, unsigned long long v) {
    // (the load spares the read-modify-write where it cannot lower the word: late rounds have few labels and many lanes)
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v)
        __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void orient_init_k(OrientState s, const uint32_t* __restrict__ orig, uint32_t n) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t == 0) s.n_edges[0] = 0;
    if (t >= n) return;
    s.parent[t] = t;
    s.comp[t] = t;
    s.slot_of[orig[t]] = t;
    s.best_u[t] = kOrientNone;
    s.best_d2[t] = 0.0;
    s.dead[t] = 0;
    s.min_d2[t] = kOrientNoKey;
    s.min_e[t] = kOrientNoKey;
    if (t + 1 < n) {
        s.edges[2 * t] = 0;
        s.edges[2 * t + 1] = 0;
    }
}

__global__ __launch_bounds__(256) void orient_scan_k(GridDesc g, const uint32_t* __restrict__ cell_start,
                                                     const double* __restrict__ qx, const double* __restrict__ qy,
                                                     const double* __restrict__ qz, const uint32_t* __restrict__ orig,
                                                     const uint32_t* __restrict__ comp, uint32_t* __restrict__ dead,
                                                     uint32_t* __restrict__ best_u, double* __restrict__ best_d2,
                                                     unsigned long long* min_d2, uint32_t n) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n || dead[t]) return;   // (a dead slot's best_u stays kOrientNone)
    const uint32_t i = orig[t], ci = comp[t];
    uint32_t bu = kOrientNone, blo = 0, bhi = 0;
    double bd = 0.0;
    prox_scan_block(g, cell_start, qx, qy, qz, t, [&](uint32_t u, double d2) {
        if (!(d2 < g.r2) || comp[u] == ci) return;   // rule O1: strictly inside the radius (t itself carries ci)
        if (bu != kOrientNone && d2 > bd) return;
        const uint32_t j = orig[u], lo = min(i, j), hi = max(i, j);
        if (bu == kOrientNone || d2 < bd || lo < blo || (lo == blo && hi < bhi)) {
            bu = u;
            bd = d2;
            blo = lo;
            bhi = hi;
        }
    });
    best_u[t] = bu;
    best_d2[t] = bd;
    if (bu == kOrientNone) dead[t] = 1;
    else atomic_min_u64(min_d2 + ci, (unsigned long long)__double_as_longlong(bd));
}

__global__ __launch_bounds__(256) void orient_pick_k(const uint32_t* __restrict__ orig, const uint32_t* __restrict__ comp,
                                                     const uint32_t* __restrict__ best_u, const double* __restrict__ best_d2,
                                                     const unsigned long long* __restrict__ min_d2, unsigned long long* min_e,
                                                     uint32_t n) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    const uint32_t u = best_u[t];
    if (u == kOrientNone) return;
    const uint32_t ci = comp[t];
    if ((unsigned long long)__double_as_longlong(best_d2[t]) != min_d2[ci]) return;
    const uint32_t i = orig[t], j = orig[u];
    atomic_min_u64(min_e + ci, ((unsigned long long)min(i, j) << 32) | max(i, j));
}

__global__ __launch_bounds__(256) void orient_hook_k(OrientState s, uint32_t n) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= n || s.comp[c] != c) return;
    const unsigned long long e = s.min_e[c];
    if (e == kOrientNoKey) return;
    const uint32_t lo = (uint32_t)(e >> 32), hi = (uint32_t)e;
    const uint32_t tlo = s.slot_of[lo], thi = s.slot_of[hi];
    const uint32_t clo = s.comp[tlo], chi = s.comp[thi];
    const uint32_t other = clo == c ? chi : clo;
    if (chi == c && s.min_e[other] == e) return;   // both labels chose this edge: the one that holds `hi` yields
    const uint32_t pos = __hip_atomic_fetch_add(s.n_edges, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (pos + 1 < n) {   // (a forest has at most n - 1 edges; the driver checks the count)
        s.edges[2 * pos] = lo;
        s.edges[2 * pos + 1] = hi;
    }
    uf_unite(s.parent, tlo, thi);
}

__global__ void orient_flatten_k(OrientState s, uint32_t n) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    uint32_t x = t;
    for (uint32_t p = s.parent[x]; p != x; p = s.parent[x]) x = p;   // (the hook launch has ended: plain loads)
    s.comp[t] = x;
    s.min_d2[t] = kOrientNoKey;
    s.min_e[t] = kOrientNoKey;
}

inline uint32_t blocks(uint32_t n) { return (n + 255) / 256; }

}  // namespace

void launch_orient_init(const OrientState& s, const uint32_t* orig, uint32_t n, hipStream_t st) {
    if (n) orient_init_k<<<blocks(n), 256, 0, st>>>(s, orig, n);
}
void launch_orient_scan(const GridDesc& g, const uint32_t* cell_start, const double* qx, const double* qy, const double* qz,
                        const uint32_t* orig, const OrientState& s, uint32_t n, hipStream_t st) {
    if (n) orient_scan_k<<<blocks(n), 256, 0, st>>>(g, cell_start, qx, qy, qz, orig, s.comp, s.dead, s.best_u, s.best_d2, s.min_d2, n);
}
void launch_orient_pick(const uint32_t* orig, const OrientState& s, uint32_t n, hipStream_t st) {
    if (n) orient_pick_k<<<blocks(n), 256, 0, st>>>(orig, s.comp, s.best_u, s.best_d2, s.min_d2, s.min_e, n);
}
void launch_orient_hook(const OrientState& s, uint32_t n, hipStream_t st) {
    if (n) orient_hook_k<<<blocks(n), 256, 0, st>>>(s, n);
}
void launch_orient_flatten(const OrientState& s, uint32_t n, hipStream_t st) {
    if (n) orient_flatten_k<<<blocks(n), 256, 0, st>>>(s, n);
}

}  // namespace m3d
