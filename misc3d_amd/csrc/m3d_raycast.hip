// m3d_raycast.hip -- pose_estimation::RayCastRenderer (src/ray_cast_renderer.cpp: Open3D's RaycastingScene over Embree) on
// gfx950: depth, instance and primitive maps of a list of posed triangle meshes seen by a pinhole camera at the origin.
//
// The contract is in include/misc3d_amd.h (m3d_raycast_pinhole, rules 1-5), its arithmetic in m3d_raycast_fp.hpp; the
// answer of a pixel depends on neither the hierarchy nor the traversal order (DESIGN.md "Ray casting").  Per frame:
//   1. rc_transform_k   fp64 pose x vertex rounded once to fp32, the frame's bounds, the first non-finite result
//   2. rc_morton_k      30-bit Morton code of every triangle box's centre inside those bounds
//   3. (m3d_radix_sort.hpp) the triangles sorted by code, stably: the effective key (code, position) is unique
//   4. rc_leaves_k      the sorted triangles' vertices gathered into 48-byte leaves
//   5. rc_tree_k        the binary radix tree over the sorted keys (Karras 2012), one thread per internal node
//   6. rc_refit_k       the boxes bottom-up, one arrival counter per node; min / max are exact, so the boxes are equal from run
//                       to run whichever child arrives first
//   7. rc_trace_k       one ray per lane, 8 x 8 pixels per wave, the stack in LDS
#include "m3d_raycast.hpp"

#include "m3d_raycast_fp.hpp"
#include "m3d_wave.hpp"

namespace m3d {

namespace {

inline uint32_t blocks_for(size_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

// fp32 <-> an unsigned integer of the same order (atomicMin / atomicMax of the bounds)
__device__ __forceinline__ uint32_t float_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

__device__ __forceinline__ uint32_t load_agent(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store_agent(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(64) void rc_reset_k(RayFrameState* __restrict__ states, uint32_t n, unsigned long long* __restrict__ counters) {
    for (uint32_t i = threadIdx.x; i < n; i += 64) {
        RayFrameState s;
        for (int c = 0; c < 3; ++c) {
            s.lo[c] = 0xFFFFFFFFu;
            s.hi[c] = 0u;
        }
        s.bad_vertex = 0xFFFFFFFFu;
        s.pad = 0;
        states[i] = s;
    }
    if (threadIdx.x < 2) counters[threadIdx.x] = 0ull;
}

// ---- 1. transform and bound ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rc_transform_k(const double* __restrict__ verts, const uint32_t* __restrict__ vert_mesh,
                                                      const double* __restrict__ poses, uint32_t n_vert, float* __restrict__ v32,
                                                      RayFrameState* state) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t bad = 0xFFFFFFFFu;
    if (i < n_vert) {
        float p[3];
        transform_vertex(poses + 16 * (size_t)vert_mesh[i], verts[3 * i], verts[3 * i + 1], verts[3 * i + 2], p);
        v32[3 * i] = p[0];
        v32[3 * i + 1] = p[1];
        v32[3 * i + 2] = p[2];
        if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
            for (int c = 0; c < 3; ++c) lo[c] = hi[c] = p[c];
        } else {
            bad = (uint32_t)i;
        }
    }
    // (every operand of the reductions is a number: min / max are exact, whatever the order)
    for (int c = 0; c < 3; ++c) {
        lo[c] = wave_min(lo[c]);
        hi[c] = wave_max(hi[c]);
    }
    bad = wave_min(bad);
    if ((threadIdx.x & 63) == 0) {
        for (int c = 0; c < 3; ++c) {
            if (lo[c] <= hi[c]) {
                atomicMin(&state->lo[c], float_key(lo[c]));
                atomicMax(&state->hi[c], float_key(hi[c]));
            }
        }
        if (bad != 0xFFFFFFFFu) atomicMin(&state->bad_vertex, bad);
    }
}

// ---- 2. Morton codes ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t spread10(uint32_t v) {   // 10 bits -> every third bit
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}

// The codes only shape the tree: any value in [0, 2^30) is a correct code, so nothing here is part of the contract.
__global__ __launch_bounds__(256) void rc_morton_k(const uint32_t* __restrict__ tris, const float* __restrict__ v32, uint32_t n_tri,
                                                   const RayFrameState* __restrict__ state, uint32_t* __restrict__ codes) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_tri) return;
    const uint32_t a = tris[3 * i], b = tris[3 * i + 1], c = tris[3 * i + 2];
    uint32_t q[3];
    for (int k = 0; k < 3; ++k) {
        const float x0 = v32[3 * (size_t)a + k], x1 = v32[3 * (size_t)b + k], x2 = v32[3 * (size_t)c + k];
        const float lo = rc_min(rc_min(x0, x1), x2), hi = rc_max(rc_max(x0, x1), x2);
        const float slo = key_float(state->lo[k]), shi = key_float(state->hi[k]);
        // (halved before they are added or subtracted: no overflow for any finite bounds)
        const float f = ((0.5f * lo + 0.5f * hi) - slo) * 0.5f / (0.5f * shi - 0.5f * slo) * 1024.0f;
        q[k] = f >= 0.0f ? (f < 1023.0f ? (uint32_t)f : 1023u) : 0u;   // (NaN: 0)
    }
    codes[i] = (spread10(q[0]) << 2) | (spread10(q[1]) << 1) | spread10(q[2]);
}

// ---- 4. leaves ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rc_leaves_k(const uint32_t* __restrict__ order, const uint32_t* __restrict__ tris,
                                                   const uint32_t* __restrict__ tri_geom, const uint32_t* __restrict__ tri_prim,
                                                   const float* __restrict__ v32, uint32_t n_tri, float4* __restrict__ leaf) {
    const size_t pos = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pos >= n_tri) return;
    const size_t i = order ? order[pos] : pos;
    const uint32_t w[3] = {tri_geom[i], tri_prim[i], 0u};
    for (int k = 0; k < 3; ++k) {
        const size_t v = tris[3 * i + k];
        leaf[3 * pos + k] = make_float4(v32[3 * v], v32[3 * v + 1], v32[3 * v + 2], __uint_as_float(w[k]));
    }
}

// ---- 5. the radix tree ----------------------------------------------------------------------------------------------------
// Length of the common prefix of keys i and j, the key of position p being (code[p], p): 64 bits of which the top two of
// the code and the top one of the position are always 0.  -1 outside [0, n).
__device__ __forceinline__ int rc_delta(const uint32_t* __restrict__ codes, long long n, long long i, long long j) {
    if (j < 0 || j >= n) return -1;
    const uint32_t a = codes[i], b = codes[j];
    return a != b ? __clz((int)(a ^ b)) : 32 + __clz((int)((uint32_t)i ^ (uint32_t)j));
}

// Karras 2012, one thread per internal node.  n_tri == 2 needs no case of its own: node 0 finds direction +1 (delta(0, -1)
// is -1), the range [0, 1] and the split 0, so its children are the leaves 0 and 1.  n_tri == 1 has no internal node and
// never comes here (launch_ray_build, rc_trace_k).
__global__ __launch_bounds__(256) void rc_tree_k(const uint32_t* __restrict__ codes, uint32_t n_tri, uint32_t* __restrict__ nodes,
                                                 uint32_t* __restrict__ parent) {
    const long long n = n_tri;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n - 1) return;
    const long long d = rc_delta(codes, n, i, i + 1) > rc_delta(codes, n, i, i - 1) ? 1 : -1;
    const int dmin = rc_delta(codes, n, i, i - d);
    long long lmax = 2;
    while (rc_delta(codes, n, i, i + lmax * d) > dmin) lmax *= 2;
    long long l = 0;
    for (long long t = lmax / 2; t >= 1; t /= 2)
        if (rc_delta(codes, n, i, i + (l + t) * d) > dmin) l += t;
    const long long j = i + l * d;
    const int dnode = rc_delta(codes, n, i, j);
    long long s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (rc_delta(codes, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const long long gamma = i + s * d + (d < 0 ? -1 : 0);
    const long long first = i < j ? i : j, last = i < j ? j : i;
    const uint32_t c0 = (uint32_t)(first == gamma ? (n - 1) + gamma : gamma);
    const uint32_t c1 = (uint32_t)(last == gamma + 1 ? (n - 1) + gamma + 1 : gamma + 1);
    nodes[(size_t)i * kRayNodeWords + 12] = c0;
    nodes[(size_t)i * kRayNodeWords + 13] = c1;
    parent[c0] = (uint32_t)i * 2u;
    parent[c1] = (uint32_t)i * 2u + 1u;
}

// ---- 6. boxes bottom-up ---------------------------------------------------------------------------------------------------
// A thread carries its subtree's box upwards: it stores the box into the parent's slot for that child, then adds 1 to the
// parent's counter; the first to arrive stops, the second reads the other slot and goes on with the union.  The slots
// cross workgroups inside one launch, so every store and load of them is an agent-scope atomic access (they bypass the
// CU's cache), the stores are released and waited for before the add that announces them, and the reader acquires
// after its add.
__global__ __launch_bounds__(256) void rc_refit_k(const float4* __restrict__ leaf, uint32_t n_tri, uint32_t* nodes,
                                                  const uint32_t* __restrict__ parent, uint32_t* visit) {
    const size_t pos = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pos >= n_tri) return;
    const float4 a = leaf[3 * pos], b = leaf[3 * pos + 1], c = leaf[3 * pos + 2];
    float lo[3] = {rc_min(rc_min(a.x, b.x), c.x), rc_min(rc_min(a.y, b.y), c.y), rc_min(rc_min(a.z, b.z), c.z)};
    float hi[3] = {rc_max(rc_max(a.x, b.x), c.x), rc_max(rc_max(a.y, b.y), c.y), rc_max(rc_max(a.z, b.z), c.z)};
    uint32_t cur = (n_tri - 1) + (uint32_t)pos;
    for (;;) {
        const uint32_t pw = parent[cur];
        const uint32_t par = pw >> 1, which = pw & 1u;
        uint32_t* slot = nodes + (size_t)par * kRayNodeWords + 6 * which;
        for (int k = 0; k < 3; ++k) {
            store_agent(slot + k, __float_as_uint(lo[k]));
            store_agent(slot + 3 + k, __float_as_uint(hi[k]));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t arrived = __hip_atomic_fetch_add(&visit[par], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (arrived == 0u) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const uint32_t* other = nodes + (size_t)par * kRayNodeWords + 6 * (which ^ 1u);
        for (int k = 0; k < 3; ++k) {
            lo[k] = rc_min(lo[k], __uint_as_float(load_agent(other + k)));
            hi[k] = rc_max(hi[k], __uint_as_float(load_agent(other + 3 + k)));
        }
        if (par == 0u) return;   // the root's own box is never asked for
        cur = par;
    }
}

// ---- 7. traversal ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rc_test_leaf(const float4* __restrict__ leaf, uint32_t pos, const float d[3], RayHit& best,
                                             uint32_t& best_pos, uint32_t& n_tests) {
    const float4 a = leaf[3 * (size_t)pos], b = leaf[3 * (size_t)pos + 1], c = leaf[3 * (size_t)pos + 2];
    const float v0[3] = {a.x, a.y, a.z}, v1[3] = {b.x, b.y, b.z}, v2[3] = {c.x, c.y, c.z};
    ++n_tests;
    float t;
    if (!ray_triangle(d, v0, v1, v2, &t)) return;
    const uint32_t geom = __float_as_uint(a.w), prim = __float_as_uint(b.w);
    if (ray_hit_better(t, geom, prim, best)) {
        best.t = t;
        best.geom = geom;
        best.prim = prim;
        best_pos = pos;
    }
}

// One ray per lane, a tile of kRayTile x kRayTile pixels per wave.
//
// THE STACK.  The key of a leaf is (code, position): the code has 30 significant bits, the position 31 (n_tri < 2^31), so
// rc_delta takes one of 30 + 31 = 61 values for two different keys.  It grows strictly from an internal node to an internal
// child, so a path from the root holds at most 61 internal nodes.  The loop below pushes at most one node per internal
// node it visits, the sibling of the one it descends into, and a pop drops every entry above the popped one: the stack holds
// at most one entry per internal node on the path to the current node, 61 at most.  kRayStackEntries = 64 rows of 64 lanes
// in LDS (16 KB a wave), entry e of lane l at word e * 64 + l: the lanes of a wave are on different banks.  There is no
// overflow path because there is no overflow.
__global__ __launch_bounds__(64) void rc_trace_k(const float4* __restrict__ leaf, const uint32_t* __restrict__ nodes, uint32_t n_tri,
                                                 RayCamera cam, RayOutputs out, unsigned long long* counters) {
    __shared__ uint32_t stack[kRayStackEntries * 64];
    const uint32_t lane = threadIdx.x;
    const uint32_t tiles_x = (cam.width + kRayTile - 1) / kRayTile;
    const uint32_t x = (blockIdx.x % tiles_x) * kRayTile + (lane % kRayTile);
    const uint32_t y = (blockIdx.x / tiles_x) * kRayTile + (lane / kRayTile);
    const bool valid = x < cam.width && y < cam.height;
    float d[3];
    ray_direction(x, y, cam.fx, cam.fy, cam.cx, cam.cy, d);
    RayHit best{INFINITY, kRayInvalidId, kRayInvalidId};
    uint32_t best_pos = kRayInvalidId, n_tests = 0, n_nodes = 0;
    if (valid && n_tri == 1u) {
        rc_test_leaf(leaf, 0u, d, best, best_pos, n_tests);   // a tree of one leaf has no internal node
    } else if (valid && n_tri > 1u) {
        const uint32_t first_leaf = n_tri - 1u;
        uint32_t node = 0u, sp = 0u;
        for (;;) {
            ++n_nodes;
            const uint4* w = reinterpret_cast<const uint4*>(nodes + (size_t)node * kRayNodeWords);
            const uint4 w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
            const float lo0[3] = {__uint_as_float(w0.x), __uint_as_float(w0.y), __uint_as_float(w0.z)};
            const float hi0[3] = {__uint_as_float(w0.w), __uint_as_float(w1.x), __uint_as_float(w1.y)};
            const float lo1[3] = {__uint_as_float(w1.z), __uint_as_float(w1.w), __uint_as_float(w2.x)};
            const float hi1[3] = {__uint_as_float(w2.y), __uint_as_float(w2.z), __uint_as_float(w2.w)};
            float l0, l1;
            const bool h0 = ray_box_may_hit(d, lo0, hi0, best.t, &l0);
            const bool h1 = ray_box_may_hit(d, lo1, hi1, best.t, &l1);
            const bool swap = h0 && h1 && l1 < l0;   // the nearer child first
            const uint32_t ca = swap ? w3.y : w3.x, cb = swap ? w3.x : w3.y;
            const bool ha = swap ? h1 : h0, hb = swap ? h0 : h1;
            const float lb = swap ? l0 : l1;
            uint32_t next = kRayInvalidId;
            if (ha) {
                if (ca >= first_leaf)
                    rc_test_leaf(leaf, ca - first_leaf, d, best, best_pos, n_tests);
                else
                    next = ca;
            }
            if (hb && !(lb > best.t)) {   // (the first child's leaf may have moved the best)
                if (cb >= first_leaf)
                    rc_test_leaf(leaf, cb - first_leaf, d, best, best_pos, n_tests);
                else if (next == kRayInvalidId)
                    next = cb;
                else
                    stack[(sp++) * 64 + lane] = cb;
            }
            if (next == kRayInvalidId) {
                if (sp == 0u) break;
                next = stack[(--sp) * 64 + lane];
            }
            node = next;
        }
    }
    if (valid) {
        const size_t pix = (size_t)y * cam.width + x;
        if (out.t_hit) out.t_hit[pix] = best.t;
        if (out.geom) out.geom[pix] = best.geom;
        if (out.prim) out.prim[pix] = best.prim;
        if (out.normals) {
            float n[3] = {0.0f, 0.0f, 0.0f};
            if (best_pos != kRayInvalidId) {
                const float4 a = leaf[3 * (size_t)best_pos], b = leaf[3 * (size_t)best_pos + 1], c = leaf[3 * (size_t)best_pos + 2];
                const float v0[3] = {a.x, a.y, a.z}, v1[3] = {b.x, b.y, b.z}, v2[3] = {c.x, c.y, c.z};
                triangle_normal(v0, v1, v2, n);
            }
            out.normals[3 * pix] = n[0];
            out.normals[3 * pix + 1] = n[1];
            out.normals[3 * pix + 2] = n[2];
        }
    }
    const unsigned long long nodes_sum = wave_sum((unsigned long long)n_nodes);
    const unsigned long long tests_sum = wave_sum((unsigned long long)n_tests);
    if (lane == 0) {
        atomicAdd(&counters[0], nodes_sum);
        atomicAdd(&counters[1], tests_sum);
    }
}

}  // namespace

void launch_ray_reset(RayFrameState* states, uint32_t n, unsigned long long* counters, hipStream_t st) {
    rc_reset_k<<<1, 64, 0, st>>>(states, n, counters);
}

void launch_ray_transform(const RayMeshes& m, const double* poses, float* v32, RayFrameState* state, hipStream_t st) {
    if (m.n_vert) rc_transform_k<<<blocks_for(m.n_vert, 256), 256, 0, st>>>(m.verts, m.vert_mesh, poses, m.n_vert, v32, state);
}

void launch_ray_morton(const RayMeshes& m, const float* v32, const RayFrameState* state, uint32_t* codes, hipStream_t st) {
    if (m.n_tri) rc_morton_k<<<blocks_for(m.n_tri, 256), 256, 0, st>>>(m.tris, v32, m.n_tri, state, codes);
}

void launch_ray_build(const RayMeshes& m, const RayTree& t, const uint32_t* sorted_codes, const uint32_t* order, hipStream_t st) {
    if (!m.n_tri) return;
    rc_leaves_k<<<blocks_for(m.n_tri, 256), 256, 0, st>>>(order, m.tris, m.tri_geom, m.tri_prim, t.v32, m.n_tri, t.leaf);
    if (m.n_tri < 2) return;   // one leaf: no internal node, nothing to build or refit
    rc_tree_k<<<blocks_for(m.n_tri - 1, 256), 256, 0, st>>>(sorted_codes, m.n_tri, t.nodes, t.parent);
    rc_refit_k<<<blocks_for(m.n_tri, 256), 256, 0, st>>>(t.leaf, m.n_tri, t.nodes, t.parent, t.visit);
}

void launch_ray_trace(const RayTree& t, uint32_t n_tri, const RayCamera& cam, const RayOutputs& out, unsigned long long* counters,
                      hipStream_t st) {
    const uint32_t tiles = ((cam.width + kRayTile - 1) / kRayTile) * ((cam.height + kRayTile - 1) / kRayTile);
    rc_trace_k<<<tiles, 64, 0, st>>>(t.leaf, t.nodes, n_tri, cam, out, counters);
}

}  // namespace m3d
