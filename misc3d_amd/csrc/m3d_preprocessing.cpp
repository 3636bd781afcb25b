// m3d_preprocessing.cpp -- misc3d::preprocessing (src/filter.cpp) behind the C ABI: FarthestPointSampling on the device
// (m3d_fps.hip) and CropROIPointCloud's index formula on the host.
#include "m3d_driver_internal.hpp"
#include "m3d_fps.hpp"
#include "m3d_fps_fp.hpp"

#include <atomic>

using namespace m3d;

namespace {

// m3d_bench_fps_force_path: 0 = by size, 1 = one workgroup, 2 = tile-pruned steps, 3 = the same steps without skipping
std::atomic<int> g_fps_force{0};

// The size up to which the one-workgroup launch runs (measured on the MI355X: DESIGN.md, "Farthest point sampling").
// Above it the cloud does not fit the workgroup's registers at 8 points per thread.
constexpr uint32_t kFpsCrossover = kFpsSingleMaxPoints;

struct FpsBufs {
    DevBuf aos, out, x, y, z, sx, sy, sz, orig, dist, tiles, wg, state;
    CellSort sort;
    void release() {
        for (DevBuf* b : {&aos, &out, &x, &y, &z, &sx, &sy, &sz, &orig, &dist, &tiles, &wg, &state}) b->release();
        sort.release();
    }
};

// The pruned path's layout: the finite points Hilbert-sorted into 512-point tiles (the grid of m3d_cloud_create) with
// orig = sorted -> original index and 0xFFFFFFFF in the padding slots.  *n_tiles_out; *sorted_out = false when the
// extent of the cloud does not allow the grid (an overflowing or subnormal extent): then every point, in input order, is
// in the tiles -- still exact (points with a non-finite coordinate keep dist = +inf: their d is NaN or +inf), only fewer
// tiles can be skipped.
int fps_layout(DeviceCtx* ctx, FpsBufs& B, const double* xyz, uint32_t n, uint32_t n_fin, const double* lo, const double* hi,
               uint32_t* n_tiles_out, bool* sorted_out) {
    hipStream_t st = ctx->stream;
    double ext = 0.0;
    for (int k = 0; k < 3; ++k) ext = std::max(ext, hi[k] - lo[k]);
    bool sorted = n_fin > 0 && std::isfinite(ext) && (ext == 0.0 || ext > 1e-290);
    for (int pass = 0; pass < 2; ++pass) {
        const uint32_t in_tiles = sorted ? n_fin : n;
        const uint32_t n_tiles = std::max<uint32_t>(1, (in_tiles + kFpsTilePoints - 1) / kFpsTilePoints);
        const uint32_t cap = n_tiles * kFpsTilePoints;
        RESERVE(B.sx, sizeof(double) * cap);
        RESERVE(B.sy, sizeof(double) * cap);
        RESERVE(B.sz, sizeof(double) * cap);
        RESERVE(B.orig, sizeof(uint32_t) * cap);
        RESERVE(B.dist, sizeof(double) * cap);
        RESERVE(B.tiles, sizeof(double) * kFpsTileDoubles * n_tiles);
        launch_fill_nan(B.sx.as<double>(), cap, st);
        launch_fill_nan(B.sy.as<double>(), cap, st);
        launch_fill_nan(B.sz.as<double>(), cap, st);
        HIPCHK(hipMemsetAsync(B.orig.p, 0xFF, sizeof(uint32_t) * cap, st));
        if (sorted) {
            const uint32_t n_pad = round_up(n, 256);
            RESERVE(B.x, sizeof(double) * n_pad);
            RESERVE(B.y, sizeof(double) * n_pad);
            RESERVE(B.z, sizeof(double) * n_pad);
            launch_aos_to_soa(B.aos.as<double>(), B.x.as<double>(), B.y.as<double>(), B.z.as<double>(), n, n_pad, st);
            const uint32_t bits = sort_grid_bits(n_fin);   // (the grid of m3d_cloud_create's sort)
            const GridDesc gs = hilbert_sort_desc(lo, sort_grid_inv_h(ext, bits), bits);
            if (!B.sort.reserve(n, gs.nx * gs.ny * gs.nz)) return M3D_ERR_DEVICE;
            CloudView v{B.x.as<double>(), B.y.as<double>(), B.z.as<double>(), nullptr, nullptr, nullptr, n, n_pad};
            launch_grid_build(v, gs, B.sort, B.sx.as<double>(), B.sy.as<double>(), B.sz.as<double>(), st, B.orig.as<uint32_t>());
            uint32_t placed = 0;
            HIPCHK(hipMemcpyAsync(&placed, B.sort.total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));
            if (placed != n_fin) {   // the grid left out a finite point (its cell test rounded): the input order instead
                sorted = false;
                continue;
            }
        } else {
            launch_aos_to_soa(B.aos.as<double>(), B.sx.as<double>(), B.sy.as<double>(), B.sz.as<double>(), n, cap, st);
            std::vector<uint32_t> iota(n);
            for (uint32_t i = 0; i < n; ++i) iota[i] = i;
            HIPCHK(hipMemcpyAsync(B.orig.p, iota.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, st));
            HIPCHK(hipStreamSynchronize(st));   // (iota is pageable and local)
        }
        launch_fps_tiles_init(B.sx.as<double>(), B.sy.as<double>(), B.sz.as<double>(), B.orig.as<uint32_t>(), n_tiles,
                              B.dist.as<double>(), B.tiles.as<double>(), st);
        HIPCHK(hipGetLastError());
        *n_tiles_out = n_tiles;
        *sorted_out = sorted;
        return M3D_OK;
    }
    return fail(M3D_ERR_DEVICE, "farthest_point_sampling: layout failed");
}

}  // namespace

extern "C" {

// misc3d::preprocessing::FarthestPointSampling, src/filter.cpp:13-52
int m3d_farthest_point_sampling(const double* xyz, size_t n, int64_t num_samples, int device, size_t* indices,
                                m3d_fps_stats* stats) {
    const double t0 = now_ms();
    if (stats) *stats = m3d_fps_stats{};
    if (!xyz && n) return fail(M3D_ERR_INVALID_ARG, "invalid argument");
    // the early cases of the reference, decided before any device is touched (:19-29); its `int` compared with size_t
    // sends a negative num_samples to the error as well, printed negative
    if (num_samples == 0) return M3D_OK;
    if (num_samples < 0 || (uint64_t)num_samples > (uint64_t)n)
        return fail(M3D_ERR_INVALID_ARG, "Illegal number of samples: " + std::to_string(num_samples) +
                                             ", must <= point size: " + std::to_string(n));
    if (!indices) return fail(M3D_ERR_INVALID_ARG, "invalid argument");
    const size_t S = (size_t)num_samples;
    if (S == n) {
        for (size_t i = 0; i < n; ++i) indices[i] = i;
        if (stats) stats->ms_total = now_ms() - t0;
        return M3D_OK;
    }
    if (n >= ((size_t)1 << 31)) return fail(M3D_ERR_INVALID_ARG, "too many points");
    // here 1 <= S < n.  One host pass: the finite points' box and number, the lowest index with a non-finite coordinate
    uint32_t nf_idx = 0xFFFFFFFFu, n_fin = 0;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = 0; i < n; ++i) {
        const double* p = xyz + 3 * i;
        if (std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2])) {
            ++n_fin;
            for (int k = 0; k < 3; ++k) {
                lo[k] = std::min(lo[k], p[k]);
                hi[k] = std::max(hi[k], p[k]);
            }
        } else if (nf_idx == 0xFFFFFFFFu) {
            nf_idx = (uint32_t)i;
        }
    }
    if (nf_idx == 0) {
        // Index 0 comes first and has a non-finite coordinate: every d is NaN or +inf, so no distance ever drops below
        // its initial +inf, and the first index of the maximum -- 0 itself -- is selected again at every step.
        for (size_t i = 0; i < S; ++i) indices[i] = 0;
        if (stats) stats->ms_total = now_ms() - t0;
        return M3D_OK;
    }
    const int force = g_fps_force.load();
    int path = force ? force : ((uint32_t)n <= kFpsCrossover ? M3D_FPS_PATH_SINGLE : M3D_FPS_PATH_PRUNED);
    if (path < M3D_FPS_PATH_SINGLE || path > M3D_FPS_PATH_DENSE) return fail(M3D_ERR_INVALID_ARG, "invalid forced path");
    if (path == M3D_FPS_PATH_SINGLE && n > kFpsSingleMaxPoints)
        return fail(M3D_ERR_INVALID_ARG, "the one-workgroup path holds at most 8192 points");
    LaneLock lane(device);
    DeviceCtx* ctx = lane.ctx;
    if (!ctx) return M3D_ERR_DEVICE;
    FpsBufs B;
    float ms_dev = 0.0f;
    uint64_t tiles_updated = 0, tile_steps = 0;
    const int rc = [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        const uint32_t nn = (uint32_t)n;
        RESERVE(B.aos, sizeof(double) * 3 * n);
        RESERVE(B.out, sizeof(uint32_t) * S);
        HIPCHK(hipMemcpyAsync(B.aos.p, xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, st));
        uint32_t* out = B.out.as<uint32_t>();
        if (path == M3D_FPS_PATH_SINGLE) {
            HIPCHK(hipEventRecord(ctx->ev0, st));
            launch_fps_single(B.aos.as<double>(), nn, (uint32_t)S, out, st);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(ctx->ev1, st));
        } else {
            uint32_t n_tiles = 0;
            bool sorted = false;
            if (const int lr = fps_layout(ctx, B, xyz, nn, n_fin, lo, hi, &n_tiles, &sorted); lr != M3D_OK) return lr;
            RESERVE(B.wg, sizeof(double) * 2 * fps_step_grid(n_tiles));
            RESERVE(B.state, sizeof(FpsState));
            FpsState s0{};
            for (int k = 0; k < 3; ++k) s0.sel[k] = xyz[k];
            HIPCHK(hipMemcpyAsync(B.state.p, &s0, sizeof(s0), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemsetAsync(out, 0, sizeof(uint32_t), st));   // indices[0] = 0; step i writes out[i + 1]
            const bool prune = path == M3D_FPS_PATH_PRUNED;
            FpsState* state = B.state.as<FpsState>();
            HIPCHK(hipEventRecord(ctx->ev0, st));
            for (size_t i = 0; i + 1 < S; ++i)
                launch_fps_step(B.aos.as<double>(), B.sx.as<double>(), B.sy.as<double>(), B.sz.as<double>(),
                                B.orig.as<uint32_t>(), n_tiles, B.dist.as<double>(), B.tiles.as<double>(), B.wg.as<double>(),
                                state, sorted ? nf_idx : 0xFFFFFFFFu, out + 1, (uint32_t)i, prune, st);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(ctx->ev1, st));
            HIPCHK(hipMemcpyAsync(&s0, B.state.p, sizeof(s0), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));   // (s0 is pageable and local)
            tiles_updated = s0.tiles_updated;
            tile_steps = (uint64_t)n_tiles * (uint64_t)(S - 1);
        }
        std::vector<uint32_t> h(S);
        HIPCHK(hipMemcpyAsync(h.data(), out, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipEventElapsedTime(&ms_dev, ctx->ev0, ctx->ev1));
        for (size_t i = 0; i < S; ++i) {
            if (h[i] >= nn) return fail(M3D_ERR_DEVICE, "farthest_point_sampling: index out of range");
            indices[i] = h[i];
        }
        return M3D_OK;
    }();
    (void)hipStreamSynchronize(ctx->stream);
    B.release();
    if (rc == M3D_OK && stats) {
        stats->ms_total = now_ms() - t0;
        stats->ms_device = ms_dev;
        stats->path = path;
        stats->tiles_updated = tiles_updated;
        stats->tile_steps = tile_steps;
    }
    return rc;
}

// misc3d::preprocessing::CropROIPointCloud's indexing, src/filter.cpp:54-101 (host only)
int m3d_crop_roi_indices(size_t n, int width, int height, int tl_x, int tl_y, int br_x, int br_y, size_t* indices, size_t* k) {
    if (!k) return fail(M3D_ERR_INVALID_ARG, "invalid argument");
    *k = 0;
    if ((int64_t)width * (int64_t)height != (int64_t)n || width < 0 || height < 0)
        return fail(M3D_ERR_INVALID_ARG, "The size of point cloud is wrong.");   // :59-62 LogError
    const int64_t roi_w = (int64_t)br_x - tl_x, roi_h = (int64_t)br_y - tl_y;
    if (roi_w <= 0) return fail(M3D_ERR_INVALID_ARG, "crop_roi: br_x must be > tl_x (the reference divides by br_x - tl_x)");
    if (roi_h < -1) return fail(M3D_ERR_INVALID_ARG, "crop_roi: br_y must be >= tl_y - 1");
    const int64_t size = (roi_w + 1) * (roi_h + 1);   // (the reference's count: rows roi_w wide, (w + 1) (h + 1) points)
    for (int64_t i = 0; i < size; ++i) {
        const int64_t ind = (i / roi_w + tl_y) * (int64_t)width + (i % roi_w) + tl_x;
        if (ind < 0 || ind >= (int64_t)n)
            return fail(M3D_ERR_INVALID_ARG, "crop_roi: the region reaches point " + std::to_string(ind) +
                                                 " outside the cloud of " + std::to_string(n) + " points");
        if (indices) indices[i] = (size_t)ind;
    }
    *k = (size_t)size;
    return M3D_OK;
}

// test / measurement hook (include/misc3d_amd_bench.h)
int m3d_bench_fps_force_path(int path) {
    if (path < 0 || path > M3D_FPS_PATH_DENSE) return fail(M3D_ERR_INVALID_ARG, "path: 0 = by size, 1 = single, 2 = pruned, 3 = dense");
    g_fps_force.store(path);
    return M3D_OK;
}

}  // extern "C"
