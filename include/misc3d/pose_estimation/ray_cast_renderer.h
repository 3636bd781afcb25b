// misc3d/pose_estimation/ray_cast_renderer.h -- pose_estimation::RayCastRenderer of the reference
// (include/misc3d/pose_estimation/ray_cast_renderer.h, src/ray_cast_renderer.cpp) over the C ABI (m3d_raycast_pinhole).
// Header-only; neither Eigen nor Open3D is needed: meshes are misc3d::TriangleMesh below (the member names of Open3D's class),
// poses row-major misc3d::Matrix4d, the maps plain vectors.  The contract -- t_hit is the z-depth, ties go to the lowest
// geometry id and then the lowest triangle index, poses are applied in double precision -- is in include/misc3d_amd.h.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../geometry.h"
#include "../logging.h"

namespace misc3d {

using Vector3i = std::array<int, 3>;

struct TriangleMesh {   // open3d::geometry::TriangleMesh's two members that matter here
    std::vector<Vector3d> vertices_;
    std::vector<Vector3i> triangles_;
};

namespace pose_estimation {

class RayCastRenderer {
public:
    // the pinhole intrinsics of open3d::camera::PinholeCameraIntrinsic(width, height, fx, fy, cx, cy)
    RayCastRenderer(int width, int height, double fx, double fy, double cx, double cy, int device = 0)
        : width_(width), height_(height), fx_(fx), fy_(fy), cx_(cx), cy_(cy), device_(device) {}

    // false (after the warning "No mesh is provided.") for an empty list; LogError when the two lists differ in length or
    // an argument is refused (m3d_raycast_pinhole, rule 5)
    bool CastRays(const std::vector<TriangleMesh>& mesh_list, const std::vector<Matrix4d>& pose_list) {
        static_assert(sizeof(Vector3i) == 3 * sizeof(int32_t) && sizeof(Vector3d) == 3 * sizeof(double), "contiguous rows");
        if (mesh_list.empty()) {
            LogWarning("No mesh is provided.");
            return false;
        }
        std::vector<m3d_raycast_mesh> meshes(mesh_list.size());
        for (size_t g = 0; g < mesh_list.size(); ++g) {
            const TriangleMesh& m = mesh_list[g];
            meshes[g].vertices = m.vertices_.empty() ? nullptr : m.vertices_[0].data();
            meshes[g].n_vertices = m.vertices_.size();
            meshes[g].triangles = m.triangles_.empty() ? nullptr : reinterpret_cast<const int32_t*>(m.triangles_[0].data());
            meshes[g].n_triangles = m.triangles_.size();
        }
        const size_t n = width_ > 0 && height_ > 0 ? (size_t)width_ * (size_t)height_ : 0;
        std::vector<float> t(n), nrm(3 * n);
        std::vector<uint32_t> geom(n), prim(n);
        CheckStatus(m3d_raycast_pinhole(meshes.data(), meshes.size(), pose_list.empty() ? nullptr : pose_list[0].data(),
                                        pose_list.size(), 1, width_, height_, fx_, fy_, cx_, cy_, device_, t.data(), geom.data(),
                                        prim.data(), nrm.data(), nullptr));
        t_hit_.swap(t);
        normals_.swap(nrm);
        geometry_ids_.swap(geom);
        primitive_ids_.swap(prim);
        num_instance_ = mesh_list.size();
        has_result_ = true;
        return true;
    }

    // height x width, row-major: t_hit (+inf where nothing is hit) and the geometry ids (0xFFFFFFFF there); empty, after the
    // warning "No ray cast result is available.", before the first cast
    std::vector<float> GetDepthMap() const { return Available() ? t_hit_ : std::vector<float>(); }
    std::vector<uint32_t> GetInstanceMap() const { return Available() ? geometry_ids_ : std::vector<uint32_t>(); }
    std::vector<uint32_t> GetPrimitiveIds() const { return Available() ? primitive_ids_ : std::vector<uint32_t>(); }

    // points = ray direction * t_hit in single precision (as the reference's tensors) widened to double, with the primitive
    // normals, in ascending pixel order: the pixels that hit anything
    PointCloud GetPointCloud() const {
        if (!Available()) return PointCloud();
        return Cloud([&](size_t i) { return std::isfinite(t_hit_[i]); });
    }
    // ... and, per mesh of the last cast, the pixels whose geometry id is that mesh's
    std::vector<PointCloud> GetInstancePointCloud() const {
        std::vector<PointCloud> out;
        if (!Available()) return out;
        out.reserve(num_instance_);
        for (size_t g = 0; g < num_instance_; ++g) out.push_back(Cloud([&](size_t i) { return geometry_ids_[i] == g; }));
        return out;
    }

private:
    bool Available() const {
        if (!has_result_) LogWarning("No ray cast result is available.");
        return has_result_;
    }
    template <class Keep>
    PointCloud Cloud(Keep keep) const {
        PointCloud pc;
        for (int y = 0; y < height_; ++y)
            for (int x = 0; x < width_; ++x) {
                const size_t i = (size_t)y * (size_t)width_ + (size_t)x;
                if (!keep(i)) continue;
                const float d[3] = {(float)((((double)x + 0.5) - cx_) / fx_), (float)((((double)y + 0.5) - cy_) / fy_), 1.0f};
                const float t = t_hit_[i];
                pc.points_.push_back({(double)(d[0] * t), (double)(d[1] * t), (double)(d[2] * t)});
                pc.normals_.push_back({(double)normals_[3 * i], (double)normals_[3 * i + 1], (double)normals_[3 * i + 2]});
            }
        return pc;
    }

    int width_, height_;
    double fx_, fy_, cx_, cy_;
    int device_;
    bool has_result_ = false;
    size_t num_instance_ = 0;
    std::vector<float> t_hit_, normals_;
    std::vector<uint32_t> geometry_ids_, primitive_ids_;
};

}  // namespace pose_estimation
}  // namespace misc3d
