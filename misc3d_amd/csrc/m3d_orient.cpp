// m3d_orient.cpp -- m3d_orient_normals_mst behind the C ABI: the radius grid ProximityExtractor builds (radius_graph_grid),
// the Boruvka rounds of m3d_orient.hip until a round adds no edge, and the host's breadth-first pass over the tree
// (m3d_ppf_train.hpp) that gives parent[] and the signs.  The contract is the block "PPF model preprocessing" of
// include/misc3d_amd.h, rules O1 - O5.
#include "m3d_driver_internal.hpp"
#include "m3d_orient.hpp"
#include "m3d_ppf_train.hpp"

#pragma clang fp contract(off)

using namespace m3d;

namespace {

struct OrientBufs {
    CellSort grid;
    DevBuf qx, qy, qz, cell_orig, parent, comp, slot_of, best_u, best_d2, dead, min_d2, min_e, edges, n_edges;
    void release() {
        grid.release();
        for (DevBuf* b : {&qx, &qy, &qz, &cell_orig, &parent, &comp, &slot_of, &best_u, &best_d2, &dead, &min_d2, &min_e, &edges, &n_edges})
            b->release();
    }
};

int orient_rounds(DeviceCtx* ctx, OrientBufs& B, const m3d_cloud* c, double radius, std::vector<uint32_t>* edges, uint64_t* rounds,
                  double* ms_grid, double* ms_rounds) {
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint32_t n = c->n;
    const double t0 = now_ms();
    GridDesc g;
    if (const int rg = radius_graph_grid(ctx, c, radius, B.grid, B.qx, B.qy, B.qz, B.cell_orig, &g); rg != M3D_OK) return rg;
    uint32_t held = 0;
    HIPCHK(hipMemcpyAsync(&held, B.grid.total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    // (every point is finite, so the grid holds every point: cell_orig is a permutation of 0 .. n - 1, which slot_of relies on)
    if (held != n) return fail(M3D_ERR_INTERNAL, "orient normals: the grid does not hold every point");
    const double t1 = now_ms();
    *ms_grid = t1 - t0;
    RESERVE(B.parent, sizeof(uint32_t) * n);
    RESERVE(B.comp, sizeof(uint32_t) * n);
    RESERVE(B.slot_of, sizeof(uint32_t) * n);
    RESERVE(B.best_u, sizeof(uint32_t) * n);
    RESERVE(B.best_d2, sizeof(double) * n);
    RESERVE(B.dead, sizeof(uint32_t) * n);
    RESERVE(B.min_d2, sizeof(uint64_t) * n);
    RESERVE(B.min_e, sizeof(uint64_t) * n);
    RESERVE(B.edges, sizeof(uint32_t) * 2 * std::max<uint32_t>(n - 1, 1));
    RESERVE(B.n_edges, 16);
    const OrientState st{B.parent.as<uint32_t>(), B.comp.as<uint32_t>(),   B.slot_of.as<uint32_t>(),
                         B.best_u.as<uint32_t>(), B.best_d2.as<double>(),  B.dead.as<uint32_t>(),
                         B.min_d2.as<unsigned long long>(), B.min_e.as<unsigned long long>(), B.edges.as<uint32_t>(),
                         B.n_edges.as<uint32_t>()};
    const uint32_t* orig = B.cell_orig.as<uint32_t>();
    launch_orient_init(st, orig, n, s);
    HIPCHK(hipGetLastError());
    uint32_t have = 0;
    *rounds = 0;
    // every round that adds an edge at least halves the number of trees that still have one: at most ceil(log2 n) of them, and
    // one more that adds none (rule O5)
    uint32_t max_rounds = 1;
    while ((1ull << (max_rounds - 1)) < n) ++max_rounds;
    for (;;) {
        if (*rounds >= max_rounds) return fail(M3D_ERR_INTERNAL, "orient normals: the rounds do not end");
        launch_orient_scan(g, B.grid.start.as<uint32_t>(), B.qx.as<double>(), B.qy.as<double>(), B.qz.as<double>(), orig, st, n, s);
        launch_orient_pick(orig, st, n, s);
        launch_orient_hook(st, n, s);
        launch_orient_flatten(st, n, s);
        HIPCHK(hipGetLastError());
        uint32_t now = 0;
        HIPCHK(hipMemcpyAsync(&now, B.n_edges.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        ++*rounds;
        if (now > n - 1) return fail(M3D_ERR_INTERNAL, "orient normals: more edges than a forest has");
        const bool grew = now != have;
        have = now;
        if (!grew || have == n - 1) break;
    }
    edges->resize(2 * (size_t)have);
    if (have) HIPCHK(hipMemcpyAsync(edges->data(), B.edges.p, sizeof(uint32_t) * 2 * have, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *ms_rounds = now_ms() - t1;
    return M3D_OK;
}

}  // namespace

int m3d::orient_normals_mst_on(DeviceCtx* ctx, const double* xyz, const double* normals, size_t n, double radius, size_t seed,
                               double* out_normals, int64_t* parent, m3d_orient_stats* stats) {
    const double t0 = now_ms();
    m3d_cloud* c = m3d_cloud_create_on(ctx, xyz, nullptr, n, 0);
    if (!c) return M3D_ERR_DEVICE;
    OrientBufs B;
    std::vector<uint32_t> edges;
    uint64_t rounds = 0;
    double ms_grid = 0.0, ms_rounds = 0.0;
    const double ms_upload = now_ms() - t0;
    const int rc = orient_rounds(ctx, B, c, radius, &edges, &rounds, &ms_grid, &ms_rounds);
    (void)hipStreamSynchronize(ctx->stream);
    B.release();
    m3d_cloud_destroy_on(c);
    if (rc != M3D_OK) return rc;
    const double t1 = now_ms();
    OrientCounts counts;
    if (!orient_tree_signs(edges.data(), edges.size() / 2, normals, n, seed, out_normals, parent, &counts))
        return fail(M3D_ERR_INTERNAL, "orient normals: a tree edge names a point outside the cloud");
    if (stats) {
        stats->rounds = rounds;
        stats->tree_edges = edges.size() / 2;
        stats->component = counts.component;
        stats->flips = counts.flips;
        stats->ms_grid = ms_upload + ms_grid;
        stats->ms_rounds = ms_rounds;
        stats->ms_signs = now_ms() - t1;
        stats->ms_total = now_ms() - t0;
    }
    return M3D_OK;
}

extern "C" int m3d_orient_normals_mst(const double* xyz, const double* normals, size_t n, double radius, size_t seed, int device,
                                      double* out_normals, int64_t* parent, m3d_orient_stats* stats) {
    if (stats) *stats = m3d_orient_stats{};
    if (!xyz || !normals || !out_normals || !parent) return fail(M3D_ERR_INVALID_ARG, "orient normals: null array");
    if (n == 0) return fail(M3D_ERR_INVALID_ARG, "orient normals: no points");
    if (n >= ((size_t)1 << 31)) return fail(M3D_ERR_INVALID_ARG, "too many points");
    if (!std::isfinite(radius) || !(radius > 0.0)) return fail(M3D_ERR_INVALID_ARG, "orient normals: the radius must be finite and > 0");
    if (seed >= n) return fail(M3D_ERR_INVALID_ARG, "orient normals: the seed is not a point of the cloud");
    for (size_t k = 0; k < 3 * n; ++k)
        if (!std::isfinite(xyz[k])) return fail(M3D_ERR_INVALID_ARG, "orient normals: point " + std::to_string(k / 3) + " is not finite");
    LaneLock lane(device);
    if (!lane.ctx) return M3D_ERR_DEVICE;
    return orient_normals_mst_on(lane.ctx, xyz, normals, n, radius, seed, out_normals, parent, stats);
}
