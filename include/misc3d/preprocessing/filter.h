// misc3d/preprocessing/filter.h -- host mirror of the reference's include/misc3d/preprocessing/filter.h
// (FarthestPointSampling, CropROIPointCloud: src/filter.cpp) over the C ABI (m3d_farthest_point_sampling,
// m3d_crop_roi_indices).  Header-only; no Eigen / Open3D needed.  ProjectIntoPlane is not on the accelerated path.
// Beside them VoxelDownSampleMulti, the multi-level form of PointCloud::VoxelDownSample (geometry.h) that MultiScaleICP
// needs (src/pipeline.cpp:937-938).
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

/**
 * @brief PointCloud::VoxelDownSample at several voxel sizes, every level computed from the ORIGINAL cloud (MultiScaleICP
 * down-samples source and target once per scale, {v, v/2, v/4}) with one upload.  Level l equals
 * pc.VoxelDownSample(voxel_sizes[l]) bit for bit.
 */
inline std::vector<PointCloud> VoxelDownSampleMulti(const PointCloud& pc, const std::vector<double>& voxel_sizes,
                                                    int device = 0) {
    const size_t n = pc.points_.size(), levels = voxel_sizes.size();
    const bool nrm = pc.HasNormals(), col = pc.HasColors();
    std::vector<PointCloud> out(levels);
    std::vector<double*> o_xyz(levels, nullptr), o_nrm(levels, nullptr), o_col(levels, nullptr);
    std::vector<size_t> m(levels, 0);
    for (size_t l = 0; l < levels; ++l) {
        out[l].points_.resize(n);
        if (nrm) out[l].normals_.resize(n);
        if (col) out[l].colors_.resize(n);
        if (n) o_xyz[l] = out[l].points_[0].data();
        if (nrm) o_nrm[l] = out[l].normals_[0].data();
        if (col) o_col[l] = out[l].colors_[0].data();
    }
    CheckStatus(m3d_voxel_down_sample_multi(n ? pc.points_[0].data() : nullptr, nrm ? pc.normals_[0].data() : nullptr,
                                            col ? pc.colors_[0].data() : nullptr, n, voxel_sizes.data(), levels, device,
                                            o_xyz.data(), o_nrm.data(), o_col.data(), nullptr, nullptr, m.data(), nullptr));
    for (size_t l = 0; l < levels; ++l) detail::voxel_shrink(out[l], m[l], nrm, col);
    return out;
}

}  // namespace preprocessing
}  // namespace misc3d
