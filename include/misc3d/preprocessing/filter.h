// misc3d/preprocessing/filter.h -- host mirror of the reference's include/misc3d/preprocessing/filter.h
// (FarthestPointSampling, CropROIPointCloud: src/filter.cpp) over the C ABI (m3d_farthest_point_sampling,
// m3d_crop_roi_indices).  Header-only; no Eigen / Open3D needed.  ProjectIntoPlane is not on the accelerated path.
#pragma once
#include <cstdint>
#include <tuple>
#include <vector>

#include <misc3d/geometry.h>
#include <misc3d/logging.h>
#include <misc3d_amd.h>

namespace misc3d {
namespace preprocessing {

/**
 * @brief Farthest point sampling of a point cloud, bit for bit the reference's: index 0 first, then the lowest index
 * of the largest distance to the samples so far.  num_samples > point count (or negative) is an error.
 */
inline std::vector<size_t> FarthestPointSampling(const CloudView& pc, int num_samples, int device = 0) {
    LogInfo("This method has been added to Open3D official branch and hence it will be deprecated in the future.");
    std::vector<size_t> indices(num_samples > 0 ? (size_t)num_samples : 0);
    CheckStatus(m3d_farthest_point_sampling(pc.xyz, pc.n, num_samples, device, indices.data(), nullptr));
    return indices;
}

/**
 * @brief Crop the region roi = (tl_x, tl_y, br_x, br_y) of an organised point cloud of shape = (width, height), with
 * the reference's indexing (rows br_x - tl_x wide, (w + 1) (h + 1) points).  Normals follow.
 */
inline PointCloud CropROIPointCloud(const PointCloud& pc, const std::tuple<int, int, int, int>& roi,
                                    const std::tuple<int, int>& shape) {
    size_t k = 0;
    const size_t n = pc.points_.size();
    CheckStatus(m3d_crop_roi_indices(n, std::get<0>(shape), std::get<1>(shape), std::get<0>(roi), std::get<1>(roi),
                                     std::get<2>(roi), std::get<3>(roi), nullptr, &k));
    std::vector<size_t> idx(k);
    CheckStatus(m3d_crop_roi_indices(n, std::get<0>(shape), std::get<1>(shape), std::get<0>(roi), std::get<1>(roi),
                                     std::get<2>(roi), std::get<3>(roi), idx.data(), &k));
    return pc.SelectByIndex(idx);
}

}  // namespace preprocessing
}  // namespace misc3d
