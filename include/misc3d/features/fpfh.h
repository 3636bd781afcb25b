// misc3d/features/fpfh.h -- host mirror of the Open3D calls the reference's registration path starts with
// (PreProcessFragments, src/pipeline.cpp:379-401; examples/cpp/transform_estimation.cpp:24-32) over the C ABI:
// EstimateNormals (unorganised clouds), ComputeFPFHFeature, and reconstruction::PreProcessFragment.  Header-only.
#pragma once
#include <vector>

#include <misc3d/features/boundary_detection.h>
#include <misc3d/geometry.h>
#include <misc3d/logging.h>
#include <misc3d/registration/correspondence_matching.h>
#include <misc3d_amd.h>

namespace misc3d {
namespace features {

// open3d::pipelines::registration::Feature: data_ is 33 x N, column-major (n rows of 33 doubles)
struct Feature {
    std::vector<double> data_;
    size_t num_ = 0;
    size_t Dimension() const { return 33; }
    size_t Num() const { return num_; }
    operator registration::FeatureView() const {  // NOLINT: implicit by design
        registration::FeatureView v;
        v.data = data_.data();
        v.dim = 33;
        v.n = num_;
        return v;
    }
};

namespace detail {
inline std::vector<Vector3d> Normals(const CloudView& pc, int search, double radius, int max_nn, const Vector3d* camera,
                                     int device) {
    std::vector<Vector3d> out(pc.n);
    const int rc = m3d_estimate_normals(pc.xyz, pc.n, search, radius, max_nn, camera ? 1 : 0, camera ? camera->data() : nullptr,
                                        device, pc.n ? out[0].data() : nullptr, nullptr);
    if (rc < 0) LogError(m3d_last_error());
    return out;
}
inline Feature Fpfh(const CloudView& pc, int search, double radius, int max_nn, int device) {
    Feature f;
    f.num_ = pc.n;
    f.data_.assign(33 * pc.n, 0.0);
    const int rc = m3d_compute_fpfh(pc.xyz, pc.normals, pc.n, search, radius, max_nn, device, f.data_.data(), nullptr);
    if (rc < 0) LogError(m3d_last_error());
    return f;
}
}  // namespace detail

// PointCloud::EstimateNormals(param); camera != nullptr: + OrientNormalsTowardsCameraLocation(*camera)
inline std::vector<Vector3d> EstimateNormals(const CloudView& pc, const KDTreeSearchParamHybrid& param,
                                             const Vector3d* camera = nullptr, int device = 0) {
    return detail::Normals(pc, 2, param.radius_, param.max_nn_, camera, device);
}
inline std::vector<Vector3d> EstimateNormals(const CloudView& pc, const KDTreeSearchParamKNN& param,
                                             const Vector3d* camera = nullptr, int device = 0) {
    return detail::Normals(pc, 0, 0.0, param.knn_, camera, device);
}
// ComputeFPFHFeature(cloud, param): the cloud must have normals
inline Feature ComputeFPFHFeature(const CloudView& pc, const KDTreeSearchParamHybrid& param, int device = 0) {
    return detail::Fpfh(pc, 2, param.radius_, param.max_nn_, device);
}
inline Feature ComputeFPFHFeature(const CloudView& pc, const KDTreeSearchParamKNN& param, int device = 0) {
    return detail::Fpfh(pc, 0, 0.0, param.knn_, device);
}

}  // namespace features

namespace reconstruction {

// PreProcessFragments for one fragment: normals (estimated when pc has none, oriented towards the origin) and FPFH
inline features::Feature PreProcessFragment(const CloudView& pc, double voxel_size, std::vector<Vector3d>* normals_out = nullptr,
                                            int device = 0) {
    features::Feature f;
    f.num_ = pc.n;
    f.data_.assign(33 * pc.n, 0.0);
    std::vector<Vector3d> nrm(pc.n);
    const int rc = m3d_preprocess_fragment(pc.xyz, pc.normals, pc.n, voxel_size, device, pc.n ? nrm[0].data() : nullptr,
                                           f.data_.data(), nullptr);
    if (rc < 0) LogError(m3d_last_error());
    if (normals_out) *normals_out = std::move(nrm);
    return f;
}

}  // namespace reconstruction
}  // namespace misc3d
