// m3d_raycast.hpp -- launchers of the ray casting kernels (m3d_raycast.hip), called by m3d_raycast.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace m3d {

constexpr uint32_t kRayTile = 8;           // a wave's rays: kRayTile x kRayTile pixels
constexpr uint32_t kRayStackEntries = 64;  // per lane, in LDS (the proof of the bound is at rc_trace_k)
constexpr uint32_t kRayNodeWords = 16;     // one internal node: 64 bytes

// what the transform of one frame leaves on the device (32 bytes)
struct RayFrameState {
    uint32_t lo[3], hi[3];   // the frame's bounds over every transformed vertex, as order-preserving integers
    uint32_t bad_vertex;     // lowest global index of a vertex whose transform is not finite in fp32, 0xFFFFFFFF if none
    uint32_t pad;
};

struct RayCamera {
    uint32_t width, height;
    double fx, fy, cx, cy;
};

// the mesh list as uploaded once; n_vert / n_tri are the totals over the list
struct RayMeshes {
    const double* verts;        // n_vert x 3
    const uint32_t* vert_mesh;  // mesh of every vertex
    const uint32_t* tris;       // n_tri x 3 global vertex indices
    const uint32_t* tri_geom;   // geometry id of every triangle
    const uint32_t* tri_prim;   // ... and its index within its mesh
    uint32_t n_vert, n_tri;
};

// one frame's hierarchy (scratch, rebuilt per frame): leaves in Morton order, n_tri - 1 internal nodes, node 0 the root;
// child ids < n_tri - 1 are internal nodes, id - (n_tri - 1) is a leaf's position otherwise
struct RayTree {
    float* v32;         // n_vert x 3: the frame's vertices
    uint32_t* codes;    // n_tri Morton codes (unsorted; the sort's input)
    float4* leaf;       // 3 per leaf: the vertices, w = geometry id / primitive id / 0 as bits
    uint32_t* nodes;    // kRayNodeWords per internal node: child 0's lo, hi, child 1's lo, hi, the child ids, 2 unused
    uint32_t* parent;   // 2 n_tri - 1: parent * 2 + which child, of every node (internal first, then the leaves)
    uint32_t* visit;    // n_tri - 1 arrival counters of the refit, zero on entry
};

struct RayOutputs {   // the frame's slices; any may be null
    float* t_hit;
    uint32_t *geom, *prim;
    float* normals;
};

// states[0 .. n): empty bounds, no bad vertex
void launch_ray_reset(RayFrameState* states, uint32_t n, unsigned long long* counters, hipStream_t st);
// rule 2 for every vertex with the frame's poses (n_mesh x 16), the bounds and the first non-finite result
void launch_ray_transform(const RayMeshes& m, const double* poses, float* v32, RayFrameState* state, hipStream_t st);
// 30-bit Morton codes of the triangle boxes' centres inside the frame's bounds
void launch_ray_morton(const RayMeshes& m, const float* v32, const RayFrameState* state, uint32_t* codes, hipStream_t st);
// the leaves in sorted order (order[pos] = triangle), the radix tree over the sorted codes, the boxes bottom-up
void launch_ray_build(const RayMeshes& m, const RayTree& t, const uint32_t* sorted_codes, const uint32_t* order, hipStream_t st);
// rules 3 and 4 for every pixel; counters[0] += nodes visited, counters[1] += pair tests
void launch_ray_trace(const RayTree& t, uint32_t n_tri, const RayCamera& cam, const RayOutputs& out, unsigned long long* counters,
                      hipStream_t st);

}  // namespace m3d
