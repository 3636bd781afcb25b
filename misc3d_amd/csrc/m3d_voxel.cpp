// m3d_voxel.cpp -- open3d::geometry::PointCloud::VoxelDownSample behind the C ABI (m3d_voxel_down_sample,
// m3d_voxel_down_sample_multi): one upload of the cloud, the bounds once, then per level keys, grouping, ordered sums
// (m3d_voxel.hip) and one download of the level's rows.  The contract is in include/misc3d_amd.h and DESIGN.md
// "Voxel down-sampling".  Nothing here depends on M3D_FP_ORDER (no sum of more than two operands).
#include "m3d_driver_internal.hpp"
#include "m3d_voxel.hpp"

#include <atomic>
#include <climits>
#include <optional>

using namespace m3d;

namespace {

// m3d_bench_voxel_force_path: 0 = by the key widths, M3D_VOXEL_PATH_PACKED, M3D_VOXEL_PATH_WIDE
std::atomic<int> g_voxel_force{0};

constexpr size_t kVoxelMaxPoints = (size_t)1 << 30;   // the hash table has 2 n slots at least, indexed by uint32

struct VoxelBufs {
    DevBuf xyz, nrm, col, bpart, bounds, key, table, first, slot, rank, vid, fidx, scan, total, k0, k1, v0, v1, counts, offs,
        oxyz, onrm, ocol;
    void release() {
        for (DevBuf* b : {&xyz, &nrm, &col, &bpart, &bounds, &key, &table, &first, &slot, &rank, &vid, &fidx, &scan, &total,
                          &k0, &k1, &v0, &v1, &counts, &offs, &oxyz, &onrm, &ocol})
            b->release();
    }
};

struct TimingEvents {   // (created per call: the lanes' two timing events are not enough for three intervals)
    hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool create() {
        for (hipEvent_t& x : e)
            if (hipEventCreate(&x) != hipSuccess) return false;
        return true;
    }
    ~TimingEvents() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

uint32_t bit_width(uint32_t v) {
    uint32_t b = 0;
    while (v) {
        ++b;
        v >>= 1;
    }
    return b;
}

bool voxel_size_ok(double v) { return v > 0.0 && std::isfinite(v); }   // (false for NaN)

int voxel_size_error(double v) {
    if (v > 0.0) return fail(M3D_ERR_INVALID_ARG, "[VoxelDownSample] voxel_size is not finite.");
    return fail(M3D_ERR_INVALID_ARG, "[VoxelDownSample] voxel_size <= 0.");
}

// rules 2 and 3 of the contract on the host: the level's grid from the exact bounds, the too-small test, and how the
// three indices pack (every point's index is <= the index of the maximum: subtraction, division and floor are monotone)
int voxel_grid(const VoxelBounds& b, double v, int force, VoxelGrid* g, bool* wide) {
    const double half = v * 0.5;
    double vmax[3], ext = -INFINITY;
    for (int c = 0; c < 3; ++c) {
        g->vmin[c] = b.lo[c] - half;
        vmax[c] = b.hi[c] + half;
        const double e = vmax[c] - g->vmin[c];
        ext = e > ext ? e : ext;
    }
    if (v * (double)INT_MAX < ext) return fail(M3D_ERR_INVALID_ARG, "[VoxelDownSample] voxel_size is too small.");
    if (!std::isfinite(ext)) return fail(M3D_ERR_INVALID_ARG, "[VoxelDownSample] the voxel bounds are not finite.");
    g->voxel_size = v;
    uint32_t sum = 0;
    for (int c = 0; c < 3; ++c) {
        const double q = std::floor((b.hi[c] - g->vmin[c]) / v);
        if (!(q >= 0.0 && q <= (double)INT_MAX)) return fail(M3D_ERR_INTERNAL, "voxel_down_sample: voxel index out of range");
        g->bits[c] = bit_width((uint32_t)q);
        sum += g->bits[c];
    }
    *wide = sum > 63 || force == M3D_VOXEL_PATH_WIDE;
    return M3D_OK;
}

struct LevelOut {
    double *xyz, *normals, *colors;
    size_t *first_index, *point_to_voxel;
};

// held: the lane of a caller that already holds one (m3d::voxel_levels_on), else the call takes a lane of `device`.
// level_ms (may be null): host clock of every level, the upload and the bounds counted with level 0
int voxel_impl(const double* xyz, const double* normals, const double* colors, size_t n, const double* voxel_sizes,
               size_t n_levels, int device, const LevelOut* outs, size_t* m_out, m3d_voxel_stats* stats,
               DeviceCtx* held = nullptr, double* level_ms = nullptr) {
    const double t0 = now_ms();
    if (level_ms)
        for (size_t l = 0; l < n_levels; ++l) level_ms[l] = 0.0;
    if (stats) *stats = m3d_voxel_stats{};
    if (!m_out || (n_levels && (!voxel_sizes || !outs))) return fail(M3D_ERR_INVALID_ARG, "invalid argument");
    for (size_t l = 0; l < n_levels; ++l) m_out[l] = 0;
    for (size_t l = 0; l < n_levels; ++l)
        if (!voxel_size_ok(voxel_sizes[l])) return voxel_size_error(voxel_sizes[l]);
    if (n == 0 || n_levels == 0) {
        if (stats) stats->ms_total = now_ms() - t0;
        return M3D_OK;
    }
    if (!xyz) return fail(M3D_ERR_INVALID_ARG, "invalid argument");
    for (size_t l = 0; l < n_levels; ++l)
        if (!outs[l].xyz || (normals && !outs[l].normals) || (colors && !outs[l].colors))
            return fail(M3D_ERR_INVALID_ARG, "invalid argument");
    if (n > kVoxelMaxPoints) return fail(M3D_ERR_INVALID_ARG, "too many points");
    const int force = g_voxel_force.load();
    std::optional<LaneLock> lane;
    if (!held) lane.emplace(device);
    DeviceCtx* ctx = held ? held : lane->ctx;
    if (!ctx) return M3D_ERR_DEVICE;
    VoxelBufs B;
    TimingEvents ev;
    float ms_up = 0.0f, ms_dev = 0.0f, ms_down = 0.0f;
    uint64_t voxels = 0;
    int path = 0, passes_total = 0;
    const int rc = [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        if (!ev.create()) return fail(M3D_ERR_DEVICE, "voxel_down_sample: hipEventCreate failed");
        hipStream_t st = ctx->stream;
        const uint32_t nn = (uint32_t)n;
        const size_t bytes3 = sizeof(double) * 3 * n;
        // ---- one upload, the bounds once
        RESERVE(B.xyz, bytes3);
        if (normals) RESERVE(B.nrm, bytes3);
        if (colors) RESERVE(B.col, bytes3);
        RESERVE(B.bpart, sizeof(VoxelBounds) * kVoxelBoundsBlocks);
        RESERVE(B.bounds, sizeof(VoxelBounds));
        HIPCHK(hipEventRecord(ev.e[0], st));
        HIPCHK(hipMemcpyAsync(B.xyz.p, xyz, bytes3, hipMemcpyHostToDevice, st));
        if (normals) HIPCHK(hipMemcpyAsync(B.nrm.p, normals, bytes3, hipMemcpyHostToDevice, st));
        if (colors) HIPCHK(hipMemcpyAsync(B.col.p, colors, bytes3, hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(ev.e[1], st));
        launch_voxel_bounds(B.xyz.as<double>(), nn, B.bpart.as<VoxelBounds>(), B.bounds.as<VoxelBounds>(), st);
        HIPCHK(hipGetLastError());
        VoxelBounds hb;
        HIPCHK(hipMemcpyAsync(&hb, B.bounds.p, sizeof(hb), hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(ev.e[2], st));
        HIPCHK(hipStreamSynchronize(st));
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms_up, ev.e[0], ev.e[1]));
        HIPCHK(hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
        ms_dev += ms;
        if (hb.first_nonfinite != kVoxelNone)
            return fail(M3D_ERR_NON_FINITE, "[VoxelDownSample] point " + std::to_string(hb.first_nonfinite) +
                                                " has a non-finite coordinate.");
        // every level's grid before any level runs: an error leaves no output half written
        std::vector<VoxelGrid> grids(n_levels);
        std::vector<char> wides(n_levels);
        for (size_t l = 0; l < n_levels; ++l) {
            bool w = false;
            if (const int gr = voxel_grid(hb, voxel_sizes[l], force, &grids[l], &w); gr != M3D_OK) return gr;
            wides[l] = w;
        }
        // ---- scratch every level uses again
        uint32_t table_size = 64;
        while ((size_t)table_size < 2 * n) table_size *= 2;
        uint32_t tile = 0, sort_blocks = 0;
        voxel_sort_shape(nn, &tile, &sort_blocks);
        const size_t n_counts = (size_t)kVoxelSortRadix * sort_blocks;
        RESERVE(B.key, sizeof(uint32_t) * 3 * n);   // (packed: 8 n bytes of it)
        RESERVE(B.table, sizeof(unsigned long long) * table_size);
        RESERVE(B.first, sizeof(uint32_t) * table_size);
        RESERVE(B.slot, sizeof(uint32_t) * n);
        RESERVE(B.rank, sizeof(uint32_t) * n);
        RESERVE(B.vid, sizeof(uint32_t) * n);
        RESERVE(B.fidx, sizeof(uint32_t) * n);
        RESERVE(B.scan, sizeof(uint32_t) * voxel_scan_scratch(std::max(n, n_counts)));
        RESERVE(B.total, 16);
        RESERVE(B.counts, sizeof(uint32_t) * n_counts);
        RESERVE(B.offs, sizeof(uint32_t) * (n + 1));
        std::vector<uint32_t> hf, hp;   // the trace on its way to the caller's size_t arrays
        double t_level = t0;
        for (size_t l = 0; l < n_levels; ++l) {
            const bool wide = wides[l] != 0;
            path = wide ? M3D_VOXEL_PATH_WIDE : M3D_VOXEL_PATH_PACKED;
            HIPCHK(hipEventRecord(ev.e[2], st));
            // keys, the hash table, the voxels ranked by their lowest member
            launch_voxel_keys(B.xyz.as<double>(), nn, grids[l], wide, B.key.as<unsigned long long>(), B.key.as<uint32_t>(), st);
            HIPCHK(hipMemsetAsync(B.table.p, 0xFF, (wide ? sizeof(uint32_t) : sizeof(unsigned long long)) * table_size, st));
            HIPCHK(hipMemsetAsync(B.first.p, 0xFF, sizeof(uint32_t) * table_size, st));
            launch_voxel_insert(nn, wide, B.key.as<unsigned long long>(), B.key.as<uint32_t>(), B.table.as<unsigned long long>(),
                                B.table.as<uint32_t>(), table_size, B.first.as<uint32_t>(), B.slot.as<uint32_t>(), st);
            launch_voxel_flags(nn, B.slot.as<uint32_t>(), B.first.as<uint32_t>(), B.rank.as<uint32_t>(), st);
            launch_scan_exclusive(B.rank.as<uint32_t>(), B.rank.as<uint32_t>(), n, B.scan.as<uint32_t>(), B.total.as<uint32_t>(), st);
            launch_voxel_ids(nn, B.slot.as<uint32_t>(), B.first.as<uint32_t>(), B.rank.as<uint32_t>(), B.vid.as<uint32_t>(),
                             B.fidx.as<uint32_t>(), st);
            HIPCHK(hipGetLastError());
            uint32_t m = 0;
            HIPCHK(hipMemcpyAsync(&m, B.total.p, sizeof(m), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));   // (m is pageable and local; the sort's passes depend on it)
            if (m == 0 || m > nn) return fail(M3D_ERR_INTERNAL, "voxel_down_sample: voxel count out of range");
            // the point indices sorted by output row, stably
            const uint32_t passes = (bit_width(m - 1) + 7) / 8;
            const uint32_t* keys = B.vid.as<uint32_t>();
            const uint32_t* vals = nullptr;
            if (passes) {
                RESERVE(B.k0, sizeof(uint32_t) * n);
                RESERVE(B.v0, sizeof(uint32_t) * n);
                if (passes > 1) {
                    RESERVE(B.k1, sizeof(uint32_t) * n);
                    RESERVE(B.v1, sizeof(uint32_t) * n);
                }
            }
            launch_radix_sort_pairs(keys, vals, nn, passes, B.k0.as<uint32_t>(), B.v0.as<uint32_t>(), B.k1.as<uint32_t>(),
                                    B.v1.as<uint32_t>(), B.counts.as<uint32_t>(), B.scan.as<uint32_t>(), B.total.as<uint32_t>(),
                                    &keys, &vals, st);
            launch_voxel_offsets(keys, nn, m, B.offs.as<uint32_t>(), st);
            // the ordered sums
            const size_t out_bytes = sizeof(double) * 3 * m;
            RESERVE(B.oxyz, out_bytes);
            if (normals) RESERVE(B.onrm, out_bytes);
            if (colors) RESERVE(B.ocol, out_bytes);
            launch_voxel_means(B.xyz.as<double>(), normals ? B.nrm.as<double>() : nullptr, colors ? B.col.as<double>() : nullptr,
                               vals, B.offs.as<uint32_t>(), m, B.oxyz.as<double>(), normals ? B.onrm.as<double>() : nullptr,
                               colors ? B.ocol.as<double>() : nullptr, st);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(ev.e[3], st));
            // one download of m rows
            const LevelOut& o = outs[l];
            HIPCHK(hipMemcpyAsync(o.xyz, B.oxyz.p, out_bytes, hipMemcpyDeviceToHost, st));
            if (normals) HIPCHK(hipMemcpyAsync(o.normals, B.onrm.p, out_bytes, hipMemcpyDeviceToHost, st));
            if (colors) HIPCHK(hipMemcpyAsync(o.colors, B.ocol.p, out_bytes, hipMemcpyDeviceToHost, st));
            if (o.first_index) {
                hf.resize(m);
                HIPCHK(hipMemcpyAsync(hf.data(), B.fidx.p, sizeof(uint32_t) * m, hipMemcpyDeviceToHost, st));
            }
            if (o.point_to_voxel) {
                hp.resize(n);
                HIPCHK(hipMemcpyAsync(hp.data(), B.vid.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
            }
            HIPCHK(hipEventRecord(ev.e[4], st));
            HIPCHK(hipStreamSynchronize(st));
            if (o.first_index)
                for (uint32_t j = 0; j < m; ++j) o.first_index[j] = hf[j];
            if (o.point_to_voxel)
                for (size_t i = 0; i < n; ++i) o.point_to_voxel[i] = hp[i];
            HIPCHK(hipEventElapsedTime(&ms, ev.e[2], ev.e[3]));
            ms_dev += ms;
            HIPCHK(hipEventElapsedTime(&ms, ev.e[3], ev.e[4]));
            ms_down += ms;
            m_out[l] = m;
            if (level_ms) {
                const double t = now_ms();
                level_ms[l] = t - t_level;
                t_level = t;
            }
            voxels += m;
            passes_total += (int)passes;
        }
        return M3D_OK;
    }();
    (void)hipStreamSynchronize(ctx->stream);
    B.release();
    if (rc != M3D_OK)
        for (size_t l = 0; l < n_levels; ++l) m_out[l] = 0;
    if (rc == M3D_OK && stats) {
        stats->ms_total = now_ms() - t0;
        stats->ms_upload = ms_up;
        stats->ms_device = ms_dev;
        stats->ms_download = ms_down;
        stats->n_voxels = voxels;
        stats->path = path;
        stats->sort_passes = passes_total;
    }
    return rc;
}

}  // namespace

// n_levels levels of one cloud on a lane the caller holds (m3d_multi_scale_icp): m3d_voxel_down_sample_multi without
// trace arrays (colours only for the coloured call), the levels' rows in the caller's host arrays
int m3d::voxel_levels_on(DeviceCtx* ctx, const double* xyz, const double* normals, size_t n, const double* voxel_sizes,
                         size_t n_levels, double* const* out_xyz, double* const* out_normals, size_t* m, double* level_ms,
                         const double* colors, double* const* out_colors) {
    std::vector<LevelOut> outs(n_levels);
    for (size_t l = 0; l < n_levels; ++l)
        outs[l] = LevelOut{out_xyz[l], out_normals ? out_normals[l] : nullptr, out_colors ? out_colors[l] : nullptr, nullptr, nullptr};
    return voxel_impl(xyz, normals, colors, n, voxel_sizes, n_levels, ctx->logical, outs.data(), m, nullptr, ctx, level_ms);
}
int m3d::voxel_sizes_check(const double* voxel_sizes, size_t n_levels) {
    for (size_t l = 0; l < n_levels; ++l)
        if (!voxel_size_ok(voxel_sizes[l])) return voxel_size_error(voxel_sizes[l]);
    return M3D_OK;
}

extern "C" {

int m3d_voxel_down_sample(const double* xyz, const double* normals, const double* colors, size_t n, double voxel_size,
                          int device, double* out_xyz, double* out_normals, double* out_colors, size_t* out_first_index,
                          size_t* point_to_voxel, size_t* m, m3d_voxel_stats* stats) {
    const LevelOut o{out_xyz, out_normals, out_colors, out_first_index, point_to_voxel};
    return voxel_impl(xyz, normals, colors, n, &voxel_size, 1, device, &o, m, stats);
}

int m3d_voxel_down_sample_multi(const double* xyz, const double* normals, const double* colors, size_t n,
                                const double* voxel_sizes, size_t n_levels, int device, double* const* out_xyz,
                                double* const* out_normals, double* const* out_colors, size_t* const* out_first_index,
                                size_t* const* point_to_voxel, size_t* m, m3d_voxel_stats* stats) {
    if (n_levels && !out_xyz) return fail(M3D_ERR_INVALID_ARG, "invalid argument");
    std::vector<LevelOut> outs(n_levels);
    for (size_t l = 0; l < n_levels; ++l)
        outs[l] = LevelOut{out_xyz[l], out_normals ? out_normals[l] : nullptr, out_colors ? out_colors[l] : nullptr,
                           out_first_index ? out_first_index[l] : nullptr, point_to_voxel ? point_to_voxel[l] : nullptr};
    return voxel_impl(xyz, normals, colors, n, voxel_sizes, n_levels, device, outs.data(), m, stats);
}

// test / measurement hook (include/misc3d_amd_bench.h)
int m3d_bench_voxel_force_path(int path) {
    if (path < 0 || path > M3D_VOXEL_PATH_WIDE) return fail(M3D_ERR_INVALID_ARG, "path: 0 = by the key widths, 1 = packed, 2 = wide");
    g_voxel_force.store(path);
    return M3D_OK;
}

}  // extern "C"
