// m3d_multi_scale_icp.cpp -- ReconstructionPipeline::MultiScaleICP (src/pipeline.cpp:927-982) as an entry point of the C ABI:
// what RegisterFragmentPair (:754-763, {voxel}, {50}) and RefineFragmentPair (:686-697, {v, v/2, v/4}, {50, 30, 15}) call.
//
//   reference, per level                                      here
//   ----------------------------------------------            -------------------------------------------------------------
//   src.VoxelDownSample(v[l]), dst.VoxelDownSample(v[l])      voxel_levels_on: one upload per cloud, every level from the original
//   RegistrationICP(.., max_dis, current, method, criteria)   registration_icp_on / registration_icp_plane_on / registration_icp_colored_on
//   GetInformationMatrixFromPointClouds (last level)          information_matrix_on on the original clouds
//
// The whole call holds ONE lane.  The levels travel through host arrays between the down-sampling and the ICP (the ICP
// entry points upload what they are given): ms_down_sample and ms_icp show what that round trip costs; keeping the levels
// resident is the open item ("Multi-scale ICP").
#include <cmath>
#include <cstring>
#include <vector>

#include "m3d_config.hpp"
#include "m3d_host_util.hpp"

using namespace m3d;

namespace {

// the colour arguments of m3d_multi_scale_icp_colored (null: one of the colourless methods)
struct ColourArgs {
    const double *src_colors, *dst_colors;
    double lambda_geometric;
};

int multi_scale_impl(const double* src, size_t n_src, const double* dst, const double* dst_normals, size_t n_dst,
                     const double* voxel_sizes, const int* max_iters, size_t n_levels, double max_correspondence_distance,
                     int method, const ColourArgs* colour, const double* T_init, int device, double* T, double* info,
                     m3d_multi_scale_icp_level* levels) {
    if (!T || !info || (!src && n_src) || (!dst && n_dst) || (n_levels && (!voxel_sizes || !max_iters)))
        return fail(M3D_ERR_INVALID_ARG, "invalid argument");
    static const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(T, T_init ? T_init : I4, sizeof(I4));
    for (int k = 0; k < 36; ++k) info[k] = 0.0;
    if (levels)
        for (size_t l = 0; l < n_levels; ++l) std::memset(&levels[l], 0, sizeof(levels[l]));
    if (n_levels == 0)   // (the reference returns an uninitialised information matrix)
        return fail(M3D_ERR_INVALID_ARG, "MultiScaleICP: no levels (voxel_sizes is empty).");
    if (!colour && (method == M3D_REFINE_COLORED_ICP || method == M3D_REFINE_GENERALIZED_ICP))
        return fail(M3D_ERR_INVALID_ARG, "MultiScaleICP: ColoredICP and GeneralizedICP are not accelerated; use "
                                         "Point2PointICP (0) or Point2PlaneICP (1).");
    if (!colour && method != M3D_REFINE_POINT2POINT_ICP && method != M3D_REFINE_POINT2PLANE_ICP)
        return fail(M3D_ERR_INVALID_ARG, "Unknown local refine method.");
    if (method != M3D_REFINE_POINT2POINT_ICP && !dst_normals) return fail(M3D_ERR_INVALID_ARG, kIcpNeedsNormals);
    if (colour && (!colour->src_colors || !colour->dst_colors)) return fail(M3D_ERR_INVALID_ARG, kIcpNeedsColors);
    if (colour && !(colour->lambda_geometric >= 0.0 && colour->lambda_geometric <= 1.0))
        return fail(M3D_ERR_INVALID_ARG, kIcpBadLambda);
    if (const int rv = voxel_sizes_check(voxel_sizes, n_levels); rv != M3D_OK) return rv;
    if (!(max_correspondence_distance > 0.0)) return fail(M3D_ERR_INVALID_ARG, kIcpInvalidDistance);
    if (n_src >= ((size_t)1 << 30) || n_dst >= ((size_t)1 << 30)) return fail(M3D_ERR_INVALID_ARG, "too many points");

    LaneLock lane(device);
    DeviceCtx* ctx = lane.ctx;
    if (!ctx) return M3D_ERR_DEVICE;
    const bool plane = method != M3D_REFINE_POINT2POINT_ICP;   // (the target's normals travel with its levels)
    // ---- every level of both clouds: one upload each
    std::vector<std::vector<double>> s_xyz(n_levels), d_xyz(n_levels), d_nrm(n_levels), s_col(n_levels), d_col(n_levels);
    std::vector<double*> ps(n_levels), pd(n_levels), pn(n_levels), pcs(n_levels, nullptr), pcd(n_levels, nullptr);
    for (size_t l = 0; l < n_levels; ++l) {
        s_xyz[l].resize(3 * std::max<size_t>(n_src, 1));
        d_xyz[l].resize(3 * std::max<size_t>(n_dst, 1));
        if (plane) d_nrm[l].resize(3 * std::max<size_t>(n_dst, 1));
        ps[l] = s_xyz[l].data();
        pd[l] = d_xyz[l].data();
        pn[l] = plane ? d_nrm[l].data() : nullptr;
        if (colour) {
            s_col[l].resize(3 * std::max<size_t>(n_src, 1));
            d_col[l].resize(3 * std::max<size_t>(n_dst, 1));
            pcs[l] = s_col[l].data();
            pcd[l] = d_col[l].data();
        }
    }
    std::vector<size_t> ms(n_levels, 0), md(n_levels, 0);
    std::vector<double> t_s(n_levels, 0.0), t_d(n_levels, 0.0);
    int rc = voxel_levels_on(ctx, src, nullptr, n_src, voxel_sizes, n_levels, ps.data(), nullptr, ms.data(), t_s.data(),
                             colour ? colour->src_colors : nullptr, colour ? pcs.data() : nullptr);
    if (rc != M3D_OK) return rc;
    rc = voxel_levels_on(ctx, dst, plane ? dst_normals : nullptr, n_dst, voxel_sizes, n_levels, pd.data(),
                         plane ? pn.data() : nullptr, md.data(), t_d.data(), colour ? colour->dst_colors : nullptr,
                         colour ? pcd.data() : nullptr);
    if (rc != M3D_OK) return rc;
    // ---- the levels, each seeded with the pose of the one before
    double current[16];
    std::memcpy(current, T, sizeof(current));
    for (size_t l = 0; l < n_levels; ++l) {
        m3d_icp_stats st;
        double next[16];
        const double t0 = now_ms();
        if (colour)
            rc = registration_icp_colored_on(ctx, ps[l], pcs[l], ms[l], pd[l], pn[l], pcd[l], md[l], max_correspondence_distance,
                                             colour->lambda_geometric, current, max_iters[l], 1e-6, 1e-6, device, next, &st,
                                             nullptr);
        else if (plane)
            rc = registration_icp_plane_on(ctx, ps[l], ms[l], pd[l], pn[l], md[l], max_correspondence_distance, current,
                                           max_iters[l], 1e-6, 1e-6, device, next, &st, nullptr, /*l1=*/false);
        else
            rc = registration_icp_on(ctx, ps[l], ms[l], pd[l], md[l], max_correspondence_distance, current, max_iters[l], 1e-6,
                                     1e-6, device, next, &st, nullptr);
        if (rc != M3D_OK) return rc;
        std::memcpy(current, next, sizeof(current));
        if (levels) {
            levels[l].n_src = ms[l];
            levels[l].n_dst = md[l];
            levels[l].icp = st;
            levels[l].ms_down_sample = t_s[l] + t_d[l];
            levels[l].ms_icp = now_ms() - t0;
        }
    }
    // ---- GetInformationMatrixFromPointClouds(src, dst, voxel_sizes[last] * 1.4, current) on the original clouds (:975-979)
    const double t1 = now_ms();
    if (n_src && n_dst) {
        m3d_cloud* csrc = m3d_cloud_create_on(ctx, src, nullptr, n_src, 0);
        if (!csrc) return M3D_ERR_DEVICE;
        m3d_cloud* cdst = m3d_cloud_create_on(ctx, dst, nullptr, n_dst, 0);
        if (!cdst) {
            m3d_cloud_destroy_on(csrc);
            return M3D_ERR_DEVICE;
        }
        rc = information_matrix_on(ctx, csrc, cdst, dst, n_dst, voxel_sizes[n_levels - 1] * 1.4, current, info, nullptr);
        m3d_cloud_destroy_on(csrc);
        m3d_cloud_destroy_on(cdst);
        if (rc != M3D_OK) return rc;
    }
    if (levels) levels[n_levels - 1].ms_information = now_ms() - t1;
    std::memcpy(T, current, sizeof(current));
    return M3D_OK;
}

}  // namespace

extern "C" int m3d_multi_scale_icp(const double* src, const double* src_normals, size_t n_src, const double* dst,
                                   const double* dst_normals, size_t n_dst, const double* voxel_sizes, const int* max_iters,
                                   size_t n_levels, double max_correspondence_distance, int method, const double* T_init,
                                   int device, double* T, double* info, m3d_multi_scale_icp_level* levels) {
    (void)src_normals;   // (no accelerated estimator reads the source's normals)
    return multi_scale_impl(src, n_src, dst, dst_normals, n_dst, voxel_sizes, max_iters, n_levels, max_correspondence_distance,
                            method, nullptr, T_init, device, T, info, levels);
}

// LocalRefineMethod::ColoredICP (src/pipeline.cpp:956-962): the levels carry the per-voxel colour means of both clouds
extern "C" int m3d_multi_scale_icp_colored(const double* src, const double* src_normals, const double* src_colors, size_t n_src,
                                           const double* dst, const double* dst_normals, const double* dst_colors, size_t n_dst,
                                           const double* voxel_sizes, const int* max_iters, size_t n_levels,
                                           double max_correspondence_distance, double lambda_geometric, const double* T_init,
                                           int device, double* T, double* info, m3d_multi_scale_icp_level* levels) {
    (void)src_normals;
    const ColourArgs colour{src_colors, dst_colors, lambda_geometric};
    return multi_scale_impl(src, n_src, dst, dst_normals, n_dst, voxel_sizes, max_iters, n_levels, max_correspondence_distance,
                            M3D_REFINE_COLORED_ICP, &colour, T_init, device, T, info, levels);
}
