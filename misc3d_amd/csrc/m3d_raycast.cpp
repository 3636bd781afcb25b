// m3d_raycast.cpp -- pose_estimation::RayCastRenderer::CastRays behind the C ABI (m3d_raycast_pinhole): the argument checks
// of rule 5, one upload of the meshes and of every frame's poses, then per frame the transform, the sort, the hierarchy and
// the traversal (m3d_raycast.hip) back to back on the lane's stream, and one download of the maps.  The contract is in
// include/misc3d_amd.h and DESIGN.md "Ray casting".
#include "m3d_driver_internal.hpp"
#include "m3d_radix_sort.hpp"
#include "m3d_raycast.hpp"
#include "m3d_raycast_fp.hpp"

using namespace m3d;

namespace {

constexpr uint64_t kRayMaxTriangles = (uint64_t)1 << 31;   // exclusive: node ids 0 .. 2 n - 2 and parent * 2 + 1 fit 32 bits
constexpr uint64_t kRayMaxVertices = (uint64_t)1 << 32;    // exclusive: 32-bit global vertex indices
constexpr uint64_t kRayMaxMeshes = 0xFFFFFFFFull;          // exclusive: 0xFFFFFFFF is the id of a miss
constexpr uint64_t kRayMaxPixels = (uint64_t)1 << 31;
constexpr uint32_t kMortonPasses = 4;                      // 30 bits, 8 a pass

struct RayBufs {
    DevBuf verts, vmesh, tris, geom, prim, poses, states, counters, v32, codes, k0, v0, k1, v1, counts, scan, total, leaf, nodes,
        parent, visit, o_t, o_g, o_p, o_n;
    void release() {
        for (DevBuf* b : {&verts, &vmesh, &tris, &geom, &prim, &poses, &states, &counters, &v32, &codes, &k0, &v0, &k1, &v1, &counts,
                          &scan, &total, &leaf, &nodes, &parent, &visit, &o_t, &o_g, &o_p, &o_n})
            b->release();
    }
};

struct EventList {
    std::vector<hipEvent_t> e;
    bool create(size_t n) {
        e.assign(n, nullptr);
        for (hipEvent_t& x : e)
            if (hipEventCreate(&x) != hipSuccess) return false;
        return true;
    }
    ~EventList() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

bool finite16(const double* T) {
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(T[k])) return false;
    return true;
}

}  // namespace

extern "C" int m3d_raycast_pinhole(const m3d_raycast_mesh* meshes, size_t n_meshes, const double* poses, size_t n_poses,
                                   size_t n_frames, int width, int height, double fx, double fy, double cx, double cy, int device,
                                   float* t_hit, uint32_t* geometry_ids, uint32_t* primitive_ids, float* primitive_normals,
                                   m3d_raycast_stats* stats) {
    const double t0 = now_ms();
    if (stats) *stats = m3d_raycast_stats{};
    // ---- rule 5, before any device work
    if (n_meshes == 0) {
        set_error("No mesh is provided.");
        return M3D_FALSE;
    }
    if (n_meshes != n_poses) return fail(M3D_ERR_SIZE_MISMATCH, "The number of meshes and poses are not matched.");
    if (!meshes || (n_frames && !poses)) return fail(M3D_ERR_INVALID_ARG, "invalid argument");
    if (width < 1 || height < 1) return fail(M3D_ERR_INVALID_ARG, "[RayCastRenderer] width and height must be at least 1.");
    if (!(std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy)))
        return fail(M3D_ERR_INVALID_ARG, "[RayCastRenderer] the intrinsic parameters are not finite.");
    if (fx == 0.0 || fy == 0.0) return fail(M3D_ERR_INVALID_ARG, "[RayCastRenderer] fx and fy must not be 0.");
    {   // the directions are monotone in x and in y: the corner pixels hold their extremes
        float d0[3], d1[3];
        ray_direction(0, 0, fx, fy, cx, cy, d0);
        ray_direction((uint32_t)width - 1, (uint32_t)height - 1, fx, fy, cx, cy, d1);
        if (!(std::isfinite(d0[0]) && std::isfinite(d0[1]) && std::isfinite(d1[0]) && std::isfinite(d1[1])))
            return fail(M3D_ERR_INVALID_ARG, "[RayCastRenderer] a ray direction is not finite in single precision.");
    }
    const uint64_t n_pix = (uint64_t)width * (uint64_t)height;
    if (n_pix >= kRayMaxPixels) return fail(M3D_ERR_INVALID_ARG, "[RayCastRenderer] too many pixels.");
    if (n_meshes >= kRayMaxMeshes) return fail(M3D_ERR_INVALID_ARG, "[RayCastRenderer] too many meshes.");
    uint64_t n_vert = 0, n_tri = 0;
    for (size_t g = 0; g < n_meshes; ++g) {
        const m3d_raycast_mesh& m = meshes[g];
        if ((m.n_vertices && !m.vertices) || (m.n_triangles && !m.triangles)) return fail(M3D_ERR_INVALID_ARG, "invalid argument");
        n_vert += m.n_vertices;
        n_tri += m.n_triangles;
        if (n_vert >= kRayMaxVertices || n_tri >= kRayMaxTriangles || m.n_vertices >= kRayMaxVertices ||
            m.n_triangles >= kRayMaxTriangles)
            return fail(M3D_ERR_INVALID_ARG, "[RayCastRenderer] too many vertices or triangles for 32-bit ids.");
    }
    for (size_t k = 0; k < n_frames * n_meshes; ++k)
        if (!finite16(poses + 16 * k))
            return fail(M3D_ERR_INVALID_ARG, "[RayCastRenderer] pose " + std::to_string(k % n_meshes) + " of frame " +
                                                 std::to_string(k / n_meshes) + " is not finite.");
    // the list flattened: global vertex indices, the mesh of every vertex, the ids of every triangle
    std::vector<uint32_t> h_tris(3 * (size_t)n_tri), h_geom((size_t)n_tri), h_prim((size_t)n_tri), h_vmesh((size_t)n_vert);
    {
        size_t vo = 0, to = 0;
        for (size_t g = 0; g < n_meshes; ++g) {
            const m3d_raycast_mesh& m = meshes[g];
            for (size_t i = 0; i < 3 * m.n_vertices; ++i)
                if (!std::isfinite(m.vertices[i]))
                    return fail(M3D_ERR_INVALID_ARG, "[RayCastRenderer] vertex " + std::to_string(i / 3) + " of mesh " +
                                                         std::to_string(g) + " is not finite.");
            for (size_t i = 0; i < m.n_vertices; ++i) h_vmesh[vo + i] = (uint32_t)g;
            for (size_t i = 0; i < m.n_triangles; ++i) {
                for (int k = 0; k < 3; ++k) {
                    const int32_t v = m.triangles[3 * i + k];
                    if (v < 0 || (uint64_t)v >= m.n_vertices)
                        return fail(M3D_ERR_INVALID_ARG, "[RayCastRenderer] triangle " + std::to_string(i) + " of mesh " +
                                                             std::to_string(g) + " has a vertex index out of range.");
                    h_tris[3 * (to + i) + k] = (uint32_t)(vo + (size_t)v);
                }
                h_geom[to + i] = (uint32_t)g;
                h_prim[to + i] = (uint32_t)i;
            }
            vo += m.n_vertices;
            to += m.n_triangles;
        }
    }
    if (n_frames == 0) {
        if (stats) stats->ms_total = now_ms() - t0;
        return M3D_OK;
    }
    if (n_frames > ((uint64_t)1 << 40) / n_pix) return fail(M3D_ERR_INVALID_ARG, "[RayCastRenderer] too many frames.");
    LaneLock lane(device);
    DeviceCtx* ctx = lane.ctx;
    if (!ctx) return M3D_ERR_DEVICE;
    RayBufs B;
    EventList ev;
    const uint32_t nt = (uint32_t)n_tri, nv = (uint32_t)n_vert;
    const size_t n_rays = (size_t)n_pix * n_frames;
    float ms_up = 0.0f, ms_build = 0.0f, ms_trace = 0.0f, ms_down = 0.0f;
    unsigned long long h_counters[2] = {0, 0};
    const int rc = [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        if (!ev.create(3 + 2 * n_frames)) return fail(M3D_ERR_DEVICE, "raycast: hipEventCreate failed");
        hipStream_t st = ctx->stream;
        // ---- the meshes and every frame's poses, once; the scratch, once
        const size_t pose_bytes = sizeof(double) * 16 * n_meshes * n_frames;
        RESERVE(B.verts, std::max<size_t>(sizeof(double) * 3 * nv, 16));
        RESERVE(B.vmesh, std::max<size_t>(sizeof(uint32_t) * nv, 16));
        RESERVE(B.tris, std::max<size_t>(sizeof(uint32_t) * 3 * nt, 16));
        RESERVE(B.geom, std::max<size_t>(sizeof(uint32_t) * nt, 16));
        RESERVE(B.prim, std::max<size_t>(sizeof(uint32_t) * nt, 16));
        RESERVE(B.poses, pose_bytes);
        RESERVE(B.states, sizeof(RayFrameState) * n_frames);
        RESERVE(B.counters, 16);
        RESERVE(B.v32, std::max<size_t>(sizeof(float) * 3 * nv, 16));
        const size_t visit_bytes = (sizeof(uint32_t) * (nt > 1 ? nt - 1 : 1) + 15) / 16 * 16;
        if (nt) {
            uint32_t tile = 0, blocks = 0;
            voxel_sort_shape(nt, &tile, &blocks);
            const size_t n_counts = (size_t)kVoxelSortRadix * blocks;
            RESERVE(B.codes, sizeof(uint32_t) * nt);
            for (DevBuf* b : {&B.k0, &B.v0, &B.k1, &B.v1}) RESERVE(*b, sizeof(uint32_t) * nt);
            RESERVE(B.counts, sizeof(uint32_t) * n_counts);
            RESERVE(B.scan, sizeof(uint32_t) * voxel_scan_scratch(n_counts));
            RESERVE(B.total, 16);
            RESERVE(B.leaf, sizeof(float4) * 3 * nt);
            RESERVE(B.nodes, sizeof(uint32_t) * kRayNodeWords * (nt > 1 ? nt - 1 : 1));
            RESERVE(B.parent, sizeof(uint32_t) * (2 * (size_t)nt - 1));
            RESERVE(B.visit, visit_bytes);
        }
        if (t_hit) RESERVE(B.o_t, sizeof(float) * n_rays);
        if (geometry_ids) RESERVE(B.o_g, sizeof(uint32_t) * n_rays);
        if (primitive_ids) RESERVE(B.o_p, sizeof(uint32_t) * n_rays);
        if (primitive_normals) RESERVE(B.o_n, sizeof(float) * 3 * n_rays);
        HIPCHK(hipEventRecord(ev.e[0], st));
        {
            size_t vo = 0;
            for (size_t g = 0; g < n_meshes; ++g) {
                if (meshes[g].n_vertices)
                    HIPCHK(hipMemcpyAsync(B.verts.as<double>() + 3 * vo, meshes[g].vertices, sizeof(double) * 3 * meshes[g].n_vertices,
                                          hipMemcpyHostToDevice, st));
                vo += meshes[g].n_vertices;
            }
        }
        if (nv) HIPCHK(hipMemcpyAsync(B.vmesh.p, h_vmesh.data(), sizeof(uint32_t) * nv, hipMemcpyHostToDevice, st));
        if (nt) {
            HIPCHK(hipMemcpyAsync(B.tris.p, h_tris.data(), sizeof(uint32_t) * 3 * nt, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(B.geom.p, h_geom.data(), sizeof(uint32_t) * nt, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(B.prim.p, h_prim.data(), sizeof(uint32_t) * nt, hipMemcpyHostToDevice, st));
        }
        HIPCHK(hipMemcpyAsync(B.poses.p, poses, pose_bytes, hipMemcpyHostToDevice, st));
        launch_ray_reset(B.states.as<RayFrameState>(), (uint32_t)n_frames, B.counters.as<unsigned long long>(), st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev.e[1], st));
        const RayMeshes M{B.verts.as<double>(), B.vmesh.as<uint32_t>(), B.tris.as<uint32_t>(), B.geom.as<uint32_t>(),
                          B.prim.as<uint32_t>(), nv, nt};
        const RayTree T{B.v32.as<float>(), B.codes.as<uint32_t>(), B.leaf.as<float4>(), B.nodes.as<uint32_t>(),
                        B.parent.as<uint32_t>(), B.visit.as<uint32_t>()};
        const RayCamera cam{(uint32_t)width, (uint32_t)height, fx, fy, cx, cy};
        // ---- the frames, back to back
        for (size_t f = 0; f < n_frames; ++f) {
            RayFrameState* state = B.states.as<RayFrameState>() + f;
            launch_ray_transform(M, B.poses.as<double>() + 16 * n_meshes * f, T.v32, state, st);
            if (nt) {
                launch_ray_morton(M, T.v32, state, T.codes, st);
                const uint32_t *sorted = nullptr, *order = nullptr;
                launch_radix_sort_pairs(T.codes, nullptr, nt, kMortonPasses, B.k0.as<uint32_t>(), B.v0.as<uint32_t>(),
                                        B.k1.as<uint32_t>(), B.v1.as<uint32_t>(), B.counts.as<uint32_t>(), B.scan.as<uint32_t>(),
                                        B.total.as<uint32_t>(), &sorted, &order, st);
                if (nt > 1) HIPCHK(hipMemsetAsync(B.visit.p, 0, visit_bytes, st));
                launch_ray_build(M, T, sorted, order, st);
            }
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(ev.e[2 + 2 * f], st));
            const RayOutputs out{t_hit ? B.o_t.as<float>() + n_pix * f : nullptr, geometry_ids ? B.o_g.as<uint32_t>() + n_pix * f : nullptr,
                                 primitive_ids ? B.o_p.as<uint32_t>() + n_pix * f : nullptr,
                                 primitive_normals ? B.o_n.as<float>() + 3 * n_pix * f : nullptr};
            launch_ray_trace(T, nt, cam, out, B.counters.as<unsigned long long>(), st);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(ev.e[3 + 2 * f], st));
        }
        // ---- one download
        std::vector<RayFrameState> h_states(n_frames);
        HIPCHK(hipMemcpyAsync(h_states.data(), B.states.p, sizeof(RayFrameState) * n_frames, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_counters, B.counters.p, sizeof(h_counters), hipMemcpyDeviceToHost, st));
        if (t_hit) HIPCHK(hipMemcpyAsync(t_hit, B.o_t.p, sizeof(float) * n_rays, hipMemcpyDeviceToHost, st));
        if (geometry_ids) HIPCHK(hipMemcpyAsync(geometry_ids, B.o_g.p, sizeof(uint32_t) * n_rays, hipMemcpyDeviceToHost, st));
        if (primitive_ids) HIPCHK(hipMemcpyAsync(primitive_ids, B.o_p.p, sizeof(uint32_t) * n_rays, hipMemcpyDeviceToHost, st));
        if (primitive_normals)
            HIPCHK(hipMemcpyAsync(primitive_normals, B.o_n.p, sizeof(float) * 3 * n_rays, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(ev.e[2 + 2 * n_frames], st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t f = 0; f < n_frames; ++f)
            if (h_states[f].bad_vertex != 0xFFFFFFFFu) {
                const uint32_t v = h_states[f].bad_vertex;
                return fail(M3D_ERR_NON_FINITE, "[RayCastRenderer] vertex " + std::to_string(v) + " of the mesh list (mesh " +
                                                    std::to_string(h_vmesh[v]) + ") is not finite in single precision under its pose of frame " +
                                                    std::to_string(f) + ".");
            }
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms_up, ev.e[0], ev.e[1]));
        for (size_t f = 0; f < n_frames; ++f) {
            HIPCHK(hipEventElapsedTime(&ms, ev.e[1 + 2 * f], ev.e[2 + 2 * f]));
            ms_build += ms;
            HIPCHK(hipEventElapsedTime(&ms, ev.e[2 + 2 * f], ev.e[3 + 2 * f]));
            ms_trace += ms;
        }
        HIPCHK(hipEventElapsedTime(&ms_down, ev.e[1 + 2 * n_frames], ev.e[2 + 2 * n_frames]));
        return M3D_OK;
    }();
    (void)hipStreamSynchronize(ctx->stream);
    B.release();
    if (rc == M3D_OK && stats) {
        stats->ms_total = now_ms() - t0;
        stats->ms_upload = ms_up;
        stats->ms_build = ms_build;
        stats->ms_traverse = ms_trace;
        stats->ms_download = ms_down;
        stats->n_triangles = n_tri;
        stats->n_nodes = n_tri ? 2 * n_tri - 1 : 0;
        stats->n_rays = n_rays;
        stats->nodes_visited = h_counters[0];
        stats->pair_tests = h_counters[1];
    }
    return rc;
}
