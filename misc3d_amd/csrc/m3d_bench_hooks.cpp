// m3d_bench_hooks.cpp -- measurement hooks of include/misc3d_amd_bench.h that need nothing of the fit's internals
// (m3d_bench_time_score / m3d_bench_plane_upper_bounds live next to issue_chunk in m3d_fit.cpp).  Not part of the boundary.
#include "m3d_driver_internal.hpp"

#pragma clang fp contract(off)

using namespace m3d;

extern "C" {

int m3d_bench_host_block(const void* p, size_t bytes) { return p && is_library_pinned(p, bytes) ? 1 : 0; }

int m3d_bench_last_segment_ms(double out[6]) {
    if (!out) return fail(M3D_ERR_INVALID_ARG, "null argument");
    for (int k = 0; k < 6; ++k) out[k] = g_seg_ms[k];
    return M3D_OK;
}

int m3d_bench_radius_grid_geom(const double lo[3], const double hi[3], double edge, int K0, int* K, double* h, uint64_t dims[3]) {
    if (!lo || !hi || !K || !h || !dims || !(edge > 0.0) || K0 < 1 || K0 > 16)
        return fail(M3D_ERR_INVALID_ARG, "invalid argument");
    const RadiusGridGeom g = radius_grid_geom(lo, hi, edge, K0);
    *K = g.K;
    *h = g.h;
    for (int k = 0; k < 3; ++k) dims[k] = g.dims[k];
    return M3D_OK;
}

int m3d_bench_reg_grid_k0(int k_cfg, uint64_t n_dst) { return reg_grid_k0(k_cfg, n_dst); }

int m3d_bench_cloud_setup_ms(const m3d_cloud* c, double out[5]) {
    if (!c || !out) return fail(M3D_ERR_INVALID_ARG, "null argument");
    for (int k = 0; k < 5; ++k) out[k] = c->setup_ms[k];
    return M3D_OK;
}

int m3d_bench_fp64_issue_rate(int device, double ms_target, double* tops, double* ms_measured) {
    if (!tops) return fail(M3D_ERR_INVALID_ARG, "invalid argument");
    LaneLock lane(device);
    DeviceCtx* ctx = lane.ctx;
    if (!ctx) return M3D_ERR_DEVICE;
    HIPCHK(hipSetDevice(ctx->device));
    RESERVE(ctx->small, 256);
    const int blocks = 256 * 8;   // 8 workgroups of 4 waves per CU: every SIMD holds 8 waves
    // one wave issues 16 * iters instructions of 4 cycles; a SIMD interleaves its 8 waves
    auto run = [&](int iters, float* ms) -> int {
        HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
        launch_fp64_issue_probe(ctx->small.as<double>(), blocks, iters, ctx->stream);
        HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
        return M3D_OK;
    };
    float ms = 0;
    int rc = run(256, &ms);   // warm-up + calibration
    if (rc != M3D_OK) return rc;
    rc = run(2048, &ms);
    if (rc != M3D_OK) return rc;
    const double per_iter = (double)ms / 2048.0;
    const int iters = (int)std::min(4.0e6, std::max(1024.0, (ms_target > 0 ? ms_target : 2.0) / std::max(per_iter, 1e-9)));
    rc = run(iters, &ms);
    if (rc != M3D_OK) return rc;
    const double ops = (double)blocks * 256.0 * 16.0 * (double)iters;
    *tops = ops / ((double)ms * 1e-3) / 1e12;
    if (ms_measured) *ms_measured = ms;
    return M3D_OK;
}

}  // extern "C"
