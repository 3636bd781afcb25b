// misc3d/reconstruction/multi_scale_icp.h -- the local-refinement stage of misc3d::reconstruction::ReconstructionPipeline
// over the C ABI: MultiScaleICP (src/pipeline.cpp:927-982) and its two callers' registration step, RefineFragmentPair
// (:686-697) and the odometry case of RegisterFragmentPair (:754-763).  Point2PointICP and Point2PlaneICP are accelerated, and
// so is ColoredICP (the reference's default) when both clouds carry colours (CloudView::colors); ColoredICP without colours and
// GeneralizedICP are refused with an error.
#pragma once
#include <array>
#include <tuple>
#include <vector>

#include "../../misc3d_amd.h"
#include "../geometry.h"
#include "../logging.h"
#include "global_registration.h"

namespace misc3d {
namespace reconstruction {

enum class LocalRefineMethod {   // PipelineConfig::LocalRefineMethod (pipeline_config.h:23-28)
    Point2PointICP = 0,
    Point2PlaneICP = 1,
    ColoredICP = 2,
    GeneralizedICP = 3
};

struct MultiScaleICPOption {
    double voxel_size = 0.01;   // PipelineConfig::voxel_size_ (a float there); max_dis = 1.4 voxel_size at every level (:936)
    LocalRefineMethod method = LocalRefineMethod::Point2PlaneICP;
    int device = 0;
    double lambda_geometric = 0.968;   // TransformationEstimationForColoredICP's (ColoredICP only)
};

// std::tuple<Eigen::Matrix4d, Eigen::Matrix6d> ReconstructionPipeline::MultiScaleICP(src, dst, voxel_size, max_iter, init_trans).
// dst needs normals for Point2PlaneICP and ColoredICP; ColoredICP runs when both views carry colours.  levels (optional): one record per level.
inline std::tuple<Matrix4d, Matrix6d> MultiScaleICP(const CloudView& src, const CloudView& dst,
                                                   const std::vector<float>& voxel_size, const std::vector<int>& max_iter,
                                                   const Matrix4d& init_trans, const MultiScaleICPOption& opt = {},
                                                   std::vector<m3d_multi_scale_icp_level>* levels = nullptr) {
    if (voxel_size.size() != max_iter.size()) LogError("one max_iter per voxel size is required");
    std::vector<double> sizes(voxel_size.begin(), voxel_size.end());   // (VoxelDownSample(double) of a float)
    if (levels) levels->assign(sizes.size(), m3d_multi_scale_icp_level{});
    Matrix4d pose;
    Matrix6d info;
    if (opt.method == LocalRefineMethod::ColoredICP && src.colors && dst.colors) {
        CheckStatus(m3d_multi_scale_icp_colored(src.xyz, src.normals, src.colors, src.n, dst.xyz, dst.normals, dst.colors, dst.n,
                                                sizes.data(), max_iter.data(), sizes.size(), (double)(float)opt.voxel_size * 1.4,
                                                opt.lambda_geometric, init_trans.data(), opt.device, pose.data(), info.data(),
                                                levels && !levels->empty() ? levels->data() : nullptr));
        return std::make_tuple(pose, info);
    }
    CheckStatus(m3d_multi_scale_icp(src.xyz, src.normals, src.n, dst.xyz, dst.normals, dst.n, sizes.data(), max_iter.data(),
                                    sizes.size(), (double)(float)opt.voxel_size * 1.4, (int)opt.method, init_trans.data(),
                                    opt.device, pose.data(), info.data(), levels && !levels->empty() ? levels->data() : nullptr));
    return std::make_tuple(pose, info);
}

// RefineFragmentPair (:686-697): {v, v / 2, v / 4} in single precision, {50, 30, 15}, seeded with the edge's pose; the
// result's pose and information are what the second pose-graph optimisation consumes.
inline void RefineFragmentPair(const CloudView& pcd_s, const CloudView& pcd_t, MatchingResult& matched_result,
                               const MultiScaleICPOption& opt = {}) {
    const float voxel_size = (float)opt.voxel_size;
    const auto result = MultiScaleICP(pcd_s, pcd_t, {voxel_size, voxel_size / 2, voxel_size / 4}, {50, 30, 15},
                                      matched_result.transformation_, opt);
    matched_result.transformation_ = std::get<0>(result);
    matched_result.information_ = std::get<1>(result);
}

// RegisterFragmentPair for adjacent fragments (:754-763): {v}, {50}, seeded with the pose from the fragment pose graph.
inline std::tuple<Matrix4d, Matrix6d> FragmentOdometry(const CloudView& pcd_s, const CloudView& pcd_t, const Matrix4d& init_trans,
                                                      const MultiScaleICPOption& opt = {}) {
    return MultiScaleICP(pcd_s, pcd_t, {(float)opt.voxel_size}, {50}, init_trans, opt);
}

}  // namespace reconstruction
}  // namespace misc3d
