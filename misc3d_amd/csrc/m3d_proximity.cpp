// m3d_proximity.cpp -- misc3d::segmentation::ProximityExtractor (src/proximity_extraction.cpp) behind the C ABI: the
// connected components of the accepted radius graph (or of the caller's neighbour lists) by a device union-find
// (m3d_proximity.hip), the evaluators' thresholds turned into exact cut-offs on the host (m3d_proximity_fp.hpp), and the
// components ordered on the host.
#include "m3d_driver_internal.hpp"
#include "m3d_proximity.hpp"
#include "m3d_proximity_fp.hpp"

#include "../../include/misc3d_amd_bench.h"

#pragma clang fp contract(off)

using namespace m3d;

// The uniform grid of detect_boundary_points' Radius search (radius_grid_geom with K0 = 1, m3d_grid_geom.hpp): cell edge 1.001
// radius, three pad cells per side, the edge doubled while the dense table would exceed 2^27 cells (a coarser cell still covers
// the radius, its 3x3x3 block only holds more points).  Points counting-sorted by cell with their original indices
// (cell_orig); grid.total[0] = the points the grid holds (those with three finite coordinates).
int m3d::radius_graph_grid(DeviceCtx* ctx, const m3d_cloud* c, double radius, CellSort& grid, DevBuf& qx, DevBuf& qy, DevBuf& qz,
                           DevBuf& cell_orig, GridDesc* g_out) {
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    if (c->bb_known)
        for (int k = 0; k < 3; ++k) {
            lo[k] = c->bb[k];
            hi[k] = c->bb[3 + k];
        }
    const double edge = radius > 0.0 ? radius : 1.0;   // (radius 0: only exact duplicates are neighbours; any cell will do)
    if (!std::isfinite(edge * 1.001)) return fail(M3D_ERR_INVALID_ARG, "proximity: search radius too large");
    const RadiusGridGeom geom = radius_grid_geom(lo, hi, edge, 1);
    if (!std::isfinite(geom.h)) return fail(M3D_ERR_INVALID_ARG, "proximity: the cloud's extent does not allow a grid");
    const GridDesc g = radius_grid_desc(geom, radius * radius, 0.0);
    const size_t n = c->n;
    if (!grid.reserve(n, g.nx * g.ny * g.nz)) return M3D_ERR_DEVICE;
    RESERVE(qx, sizeof(double) * n);
    RESERVE(qy, sizeof(double) * n);
    RESERVE(qz, sizeof(double) * n);
    RESERVE(cell_orig, sizeof(uint32_t) * n);
    launch_grid_build(c->view(), g, grid, qx.as<double>(), qy.as<double>(), qz.as<double>(), ctx->stream,
                      cell_orig.as<uint32_t>());
    HIPCHK(hipGetLastError());
    *g_out = g;
    return M3D_OK;
}

namespace {

struct ProxBufs {
    CellSort grid;
    DevBuf qx, qy, qz, cell_orig, snx, sny, snz, parent, size, root, off, idx, nb_d2;
    void release() {
        grid.release();
        for (DevBuf* b : {&qx, &qy, &qz, &cell_orig, &snx, &sny, &snz, &parent, &size, &root, &off, &idx, &nb_d2}) b->release();
    }
};

int prox_grid(DeviceCtx* ctx, ProxBufs& B, const m3d_cloud* c, double radius, GridDesc* g_out) {
    return radius_graph_grid(ctx, c, radius, B.grid, B.qx, B.qy, B.qz, B.cell_orig, g_out);
}

// Components (root[i]: the smallest index of i's component, size[r]: the size of root r's) -> the reference's output:
// min_size <= |C| <= max_size kept, size descending, ties by the root (= the smallest member) ascending, members ascending.
void prox_order(const uint32_t* root, const uint32_t* size, size_t n, size_t min_size, size_t max_size, size_t* offsets,
                size_t* indices, size_t* n_clusters, size_t* labels, uint64_t* components) {
    std::vector<uint32_t> kept;
    uint64_t comps = 0;
    for (size_t r = 0; r < n; ++r)
        if (root[r] == r) {
            ++comps;
            if (size[r] >= min_size && size[r] <= max_size) kept.push_back((uint32_t)r);
        }
    std::stable_sort(kept.begin(), kept.end(), [size](uint32_t a, uint32_t b) { return size[a] > size[b]; });
    const size_t nk = kept.size();
    std::vector<uint32_t> rank(n, 0xFFFFFFFFu);
    offsets[0] = 0;
    for (size_t k = 0; k < nk; ++k) {
        rank[kept[k]] = (uint32_t)k;
        offsets[k + 1] = offsets[k] + size[kept[k]];
    }
    std::vector<size_t> cursor(offsets, offsets + nk);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t rk = rank[root[i]];
        if (rk != 0xFFFFFFFFu) indices[cursor[rk]++] = i;
        if (labels) labels[i] = rk != 0xFFFFFFFFu ? (size_t)rk : nk;
    }
    *n_clusters = nk;
    if (components) *components = comps;
}

int check_common(const double* xyz, const double* normals, size_t n_normals, size_t n, const m3d_proximity_evaluator* ev,
                 size_t* cluster_offsets, size_t* cluster_indices, size_t* n_clusters) {
    if (!ev || !n_clusters || !cluster_offsets || (n && (!xyz || !cluster_indices)))
        return fail(M3D_ERR_INVALID_ARG, "invalid argument");
    if (ev->kind < M3D_PROX_DISTANCE || ev->kind > M3D_PROX_DISTANCE_NORMALS)
        return fail(M3D_ERR_INVALID_ARG, "proximity: unknown evaluator kind");
    if (ev->kind != M3D_PROX_DISTANCE && n && (!normals || n_normals < n))
        return fail(M3D_ERR_INVALID_ARG, "Index exceed size of data!");
    if (n >= ((size_t)1 << 31)) return fail(M3D_ERR_INVALID_ARG, "too many points");
    return M3D_OK;
}

// the common tail of both overloads: parent[] filled by the union launch(es) -> flatten -> host ordering
int prox_finish(DeviceCtx* ctx, ProxBufs& B, uint32_t n, size_t min_size, size_t max_size, size_t* offsets, size_t* indices,
                size_t* n_clusters, size_t* labels, m3d_proximity_stats* st) {
    hipStream_t s = ctx->stream;
    RESERVE(B.root, sizeof(uint32_t) * n);
    launch_prox_flatten(B.parent.as<uint32_t>(), B.root.as<uint32_t>(), B.size.as<uint32_t>(), n, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev1, s));
    std::vector<uint32_t> root(n), size(n);
    HIPCHK(hipMemcpyAsync(root.data(), B.root.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(size.data(), B.size.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    for (uint32_t i = 0; i < n; ++i)
        if (root[i] > i || root[root[i]] != root[i]) return fail(M3D_ERR_INTERNAL, "proximity: union-find self-check failed");
    const double t0 = now_ms();
    prox_order(root.data(), size.data(), n, min_size, max_size, offsets, indices, n_clusters, labels,
               st ? &st->components : nullptr);
    if (st) {
        st->ms_device = ms;
        st->ms_order = now_ms() - t0;
    }
    return M3D_OK;
}

}  // namespace

extern "C" {

// misc3d::segmentation::ProximityExtractor::Segment(pc, search_radius, evaluator), src/proximity_extraction.cpp:51-57,74-190
int m3d_proximity_segment(const double* xyz, const double* normals, size_t n_normals, size_t n, double radius,
                          const m3d_proximity_evaluator* ev, size_t min_size, size_t max_size, int device,
                          size_t* cluster_offsets, size_t* cluster_indices, size_t* n_clusters, size_t* labels,
                          m3d_proximity_stats* stats) {
    const double t0 = now_ms();
    if (stats) *stats = m3d_proximity_stats{};
    if (const int r = check_common(xyz, normals, n_normals, n, ev, cluster_offsets, cluster_indices, n_clusters); r != M3D_OK)
        return r;
    if (!std::isfinite(radius) || radius < 0.0)
        return fail(M3D_ERR_INVALID_ARG, "proximity: the search radius must be finite and >= 0");
    *n_clusters = 0;
    cluster_offsets[0] = 0;
    if (n == 0) return M3D_OK;
    const bool with_normals = ev->kind != M3D_PROX_DISTANCE;
    const ProxCut cut = prox_cut(ev->kind, ev->dist, ev->angle_deg);
    LaneLock lane(device);
    DeviceCtx* ctx = lane.ctx;
    if (!ctx) return M3D_ERR_DEVICE;
    m3d_cloud* c = m3d_cloud_create_on(ctx, xyz, with_normals ? normals : nullptr, n, 0);
    if (!c) return M3D_ERR_DEVICE;
    ProxBufs B;
    GridDesc g;
    const int rc = [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        const uint32_t nn = (uint32_t)n;
        HIPCHK(hipEventRecord(ctx->ev0, s));
        if (const int rg = prox_grid(ctx, B, c, radius, &g); rg != M3D_OK) return rg;
        const uint32_t* n_sorted = B.grid.total.as<uint32_t>();
        if (with_normals) {
            RESERVE(B.snx, sizeof(double) * n);
            RESERVE(B.sny, sizeof(double) * n);
            RESERVE(B.snz, sizeof(double) * n);
            launch_prox_gather_normals(c->view(), B.cell_orig.as<uint32_t>(), nn, n_sorted, B.snx.as<double>(),
                                       B.sny.as<double>(), B.snz.as<double>(), s);
        }
        RESERVE(B.parent, sizeof(uint32_t) * n);
        RESERVE(B.size, sizeof(uint32_t) * n);
        launch_prox_init(B.parent.as<uint32_t>(), B.size.as<uint32_t>(), nn, s);
        launch_prox_union_grid(g, B.grid.start.as<uint32_t>(), B.qx.as<double>(), B.qy.as<double>(), B.qz.as<double>(),
                               B.cell_orig.as<uint32_t>(), B.snx.as<double>(), B.sny.as<double>(), B.snz.as<double>(), nn,
                               n_sorted, cut, B.parent.as<uint32_t>(), s);
        HIPCHK(hipGetLastError());
        return prox_finish(ctx, B, nn, min_size, max_size, cluster_offsets, cluster_indices, n_clusters, labels, stats);
    }();
    (void)hipStreamSynchronize(ctx->stream);
    B.release();
    m3d_cloud_destroy_on(c);
    if (rc == M3D_OK && stats) {
        stats->ms_total = now_ms() - t0;
        stats->cell_edge = 1.0 / g.inv_h;
    }
    return rc;
}

// misc3d::segmentation::ProximityExtractor::Segment(pc, nn_indices, evaluator), src/proximity_extraction.cpp:59-72
int m3d_proximity_segment_nn(const double* xyz, const double* normals, size_t n_normals, size_t n, size_t n_lists,
                             const size_t* nn_offsets, const size_t* nn_indices, const m3d_proximity_evaluator* ev,
                             size_t min_size, size_t max_size, int device, size_t* cluster_offsets,
                             size_t* cluster_indices, size_t* n_clusters, size_t* labels, m3d_proximity_stats* stats) {
    const double t0 = now_ms();
    if (stats) *stats = m3d_proximity_stats{};
    if (const int r = check_common(xyz, normals, n_normals, n, ev, cluster_offsets, cluster_indices, n_clusters); r != M3D_OK)
        return r;
    if (n_lists != n) return fail(M3D_ERR_INVALID_ARG, "The number of input data size are not equal!");   // :63-67
    if (!nn_offsets) return fail(M3D_ERR_INVALID_ARG, "invalid argument");
    *n_clusters = 0;
    cluster_offsets[0] = 0;
    if (n == 0) return M3D_OK;
    // the lists on the host once: offsets non-decreasing, every index in [0, n) (the reference reads out of bounds there)
    const size_t total = nn_offsets[n];
    if (total && !nn_indices) return fail(M3D_ERR_INVALID_ARG, "invalid argument");
    for (size_t i = 0; i < n; ++i)
        if (nn_offsets[i] > nn_offsets[i + 1]) return fail(M3D_ERR_INVALID_ARG, "proximity: nn offsets must not decrease");
    std::vector<uint32_t> idx32(std::max<size_t>(total, 1));
    for (size_t k = 0; k < total; ++k) {
        if (nn_indices[k] >= n)
            return fail(M3D_ERR_INVALID_ARG, "proximity: neighbour index " + std::to_string(nn_indices[k]) +
                                                 " outside the cloud of " + std::to_string(n) + " points");
        idx32[k] = (uint32_t)nn_indices[k];
    }
    static_assert(sizeof(size_t) == sizeof(uint64_t), "size_t is 64 bits on this platform");
    const bool with_normals = ev->kind != M3D_PROX_DISTANCE;
    const ProxCut cut = prox_cut(ev->kind, ev->dist, ev->angle_deg);
    LaneLock lane(device);
    DeviceCtx* ctx = lane.ctx;
    if (!ctx) return M3D_ERR_DEVICE;
    m3d_cloud* c = m3d_cloud_create_on(ctx, xyz, with_normals ? normals : nullptr, n, 0);
    if (!c) return M3D_ERR_DEVICE;
    ProxBufs B;
    const int rc = [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        const uint32_t nn = (uint32_t)n;
        RESERVE(B.off, sizeof(uint64_t) * (n + 1));
        RESERVE(B.idx, sizeof(uint32_t) * idx32.size());
        HIPCHK(hipMemcpyAsync(B.off.p, nn_offsets, sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(B.idx.p, idx32.data(), sizeof(uint32_t) * idx32.size(), hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(ctx->ev0, s));
        RESERVE(B.parent, sizeof(uint32_t) * n);
        RESERVE(B.size, sizeof(uint32_t) * n);
        launch_prox_init(B.parent.as<uint32_t>(), B.size.as<uint32_t>(), nn, s);
        launch_prox_union_lists(c->view(), B.off.as<uint64_t>(), B.idx.as<uint32_t>(), nn, cut, B.parent.as<uint32_t>(), s);
        HIPCHK(hipGetLastError());
        return prox_finish(ctx, B, nn, min_size, max_size, cluster_offsets, cluster_indices, n_clusters, labels, stats);
    }();
    (void)hipStreamSynchronize(ctx->stream);
    B.release();
    m3d_cloud_destroy_on(c);
    if (rc == M3D_OK && stats) stats->ms_total = now_ms() - t0;
    return rc;
}

// radius neighbour lists for the user-evaluator path (include/misc3d_amd.h)
int m3d_radius_neighbors(const double* xyz, size_t n, double radius, int device, size_t* offsets, uint32_t* nb_indices,
                         double* nb_d2, size_t capacity, size_t* total) {
    if (!offsets || !total || (n && !xyz)) return fail(M3D_ERR_INVALID_ARG, "invalid argument");
    if (!std::isfinite(radius) || radius < 0.0)
        return fail(M3D_ERR_INVALID_ARG, "proximity: the search radius must be finite and >= 0");
    if (n >= ((size_t)1 << 31)) return fail(M3D_ERR_INVALID_ARG, "too many points");
    *total = 0;
    offsets[0] = 0;
    if (n == 0) return M3D_OK;
    LaneLock lane(device);
    DeviceCtx* ctx = lane.ctx;
    if (!ctx) return M3D_ERR_DEVICE;
    m3d_cloud* c = m3d_cloud_create_on(ctx, xyz, nullptr, n, 0);
    if (!c) return M3D_ERR_DEVICE;
    ProxBufs B;
    const int rc = [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        const uint32_t nn = (uint32_t)n;
        GridDesc g;
        if (const int rg = prox_grid(ctx, B, c, radius, &g); rg != M3D_OK) return rg;
        RESERVE(B.size, sizeof(uint32_t) * n);
        HIPCHK(hipMemsetAsync(B.size.p, 0, sizeof(uint32_t) * n, s));   // (points outside the grid have no neighbours)
        launch_prox_nb_count(g, B.grid.start.as<uint32_t>(), B.qx.as<double>(), B.qy.as<double>(), B.qz.as<double>(),
                             B.cell_orig.as<uint32_t>(), nn, B.grid.total.as<uint32_t>(), B.size.as<uint32_t>(), s);
        HIPCHK(hipGetLastError());
        std::vector<uint32_t> cnt(n);
        HIPCHK(hipMemcpyAsync(cnt.data(), B.size.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (size_t i = 0; i < n; ++i) offsets[i + 1] = offsets[i] + cnt[i];
        *total = offsets[n];
        if (!nb_indices || !nb_d2 || capacity < offsets[n]) return M3D_OK;
        RESERVE(B.off, sizeof(uint64_t) * (n + 1));
        RESERVE(B.idx, sizeof(uint32_t) * std::max<size_t>(offsets[n], 1));
        RESERVE(B.nb_d2, sizeof(double) * std::max<size_t>(offsets[n], 1));
        HIPCHK(hipMemcpyAsync(B.off.p, offsets, sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice, s));
        launch_prox_nb_fill(g, B.grid.start.as<uint32_t>(), B.qx.as<double>(), B.qy.as<double>(), B.qz.as<double>(),
                            B.cell_orig.as<uint32_t>(), nn, B.grid.total.as<uint32_t>(), B.off.as<uint64_t>(),
                            B.idx.as<uint32_t>(), B.nb_d2.as<double>(), s);
        HIPCHK(hipGetLastError());
        if (offsets[n]) {
            HIPCHK(hipMemcpyAsync(nb_indices, B.idx.p, sizeof(uint32_t) * offsets[n], hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(nb_d2, B.nb_d2.p, sizeof(double) * offsets[n], hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
        return M3D_OK;
    }();
    (void)hipStreamSynchronize(ctx->stream);
    B.release();
    m3d_cloud_destroy_on(c);
    return rc;
}

// test hook (include/misc3d_amd_bench.h)
int m3d_bench_proximity_cutoffs(double dist, double angle_deg, double out[5]) {
    if (!out) return fail(M3D_ERR_INVALID_ARG, "null argument");
    const ProxCut c = prox_cut(kProxDistanceNormals, dist, angle_deg);
    out[0] = c.d2_cut;
    out[1] = c.lo1;
    out[2] = c.hi1;
    out[3] = c.lo2;
    out[4] = c.hi2;
    return M3D_OK;
}

}  // extern "C"
