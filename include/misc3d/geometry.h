// misc3d/geometry.h -- the point-cloud types the host API accepts.
//
// The reference passes open3d::geometry::PointCloud (points_/normals_ = std::vector<Eigen::Vector3d>,
// contiguous N x 3 float64).  Open3D and Eigen are not dependencies of this implementation: the API
// takes a non-owning CloudView, constructible from misc3d::PointCloud below (same member names as
// Open3D's class) or, with MISC3D_WITH_OPEN3D defined, directly from an Open3D cloud without a copy.
#pragma once
#include "../misc3d_amd.h"

#include <array>
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#ifdef MISC3D_WITH_OPEN3D
#include <open3d/geometry/PointCloud.h>
#endif

namespace misc3d {

using Vector3d = std::array<double, 3>;
using Vector4d = std::array<double, 4>;
using Matrix4d = std::array<double, 16>;  // row-major

struct PointCloud {
    std::vector<Vector3d> points_;
    std::vector<Vector3d> normals_;
    std::vector<Vector3d> colors_;   // Open3D's: RGB in [0, 1], one per point or none
    PointCloud() = default;
    explicit PointCloud(std::vector<Vector3d> points) : points_(std::move(points)) {}
    bool HasPoints() const { return !points_.empty(); }
    bool HasNormals() const { return !points_.empty() && normals_.size() == points_.size(); }
    bool HasColors() const { return !points_.empty() && colors_.size() == points_.size(); }
    // open3d::geometry::PointCloud::SelectByIndex: order preserved, normals and colours follow
    PointCloud SelectByIndex(const std::vector<size_t>& indices, bool invert = false) const {
        PointCloud out;
        const bool nrm = HasNormals(), col = HasColors();
        if (!invert) {
            for (size_t i : indices) {
                out.points_.push_back(points_[i]);
                if (nrm) out.normals_.push_back(normals_[i]);
                if (col) out.colors_.push_back(colors_[i]);
            }
        } else {
            std::vector<char> mask(points_.size(), 0);
            for (size_t i : indices) mask[i] = 1;
            for (size_t i = 0; i < points_.size(); ++i)
                if (!mask[i]) {
                    out.points_.push_back(points_[i]);
                    if (nrm) out.normals_.push_back(normals_[i]);
                    if (col) out.colors_.push_back(colors_[i]);
                }
        }
        return out;
    }
    // open3d::geometry::PointCloud::VoxelDownSample on the device (m3d_voxel_down_sample): the per-voxel means of points,
    // normals and colours bit for bit the reference's (members added in ascending index); the voxels come in ascending
    // order of their lowest member index (the reference's order is that of an unordered_map).  Defined in
    // the end of this header.  Errors throw std::runtime_error with the reference's text.
    PointCloud VoxelDownSample(double voxel_size, int device = 0) const;
};

struct CloudView {
    const double* xyz = nullptr;      // n x 3
    const double* normals = nullptr;  // n x 3 or null
    size_t n = 0;
    const double* colors = nullptr;   // n x 3 (RGB) or null: read by coloured ICP only
    CloudView() = default;
    CloudView(const double* p, const double* nrm, size_t count) : xyz(p), normals(nrm), n(count) {}
    CloudView(const double* p, const double* nrm, const double* rgb, size_t count) : xyz(p), normals(nrm), n(count), colors(rgb) {}
    CloudView(const PointCloud& pc)  // NOLINT: implicit by design
        : xyz(pc.points_.empty() ? nullptr : pc.points_[0].data()),
          normals(pc.HasNormals() ? pc.normals_[0].data() : nullptr),
          n(pc.points_.size()),
          colors(pc.HasColors() ? pc.colors_[0].data() : nullptr) {}
#ifdef MISC3D_WITH_OPEN3D
    CloudView(const open3d::geometry::PointCloud& pc)  // NOLINT: Eigen::Vector3d is 24-byte POD
        : xyz(pc.points_.empty() ? nullptr : pc.points_[0].data()),
          normals(pc.HasNormals() ? pc.normals_[0].data() : nullptr),
          n(pc.points_.size()),
          colors(pc.HasColors() ? pc.colors_[0].data() : nullptr) {}
#endif
};

// ---- page-locked scratch of the host mirrors ---------------------------------------------------------------------------------
// Large results (index lists, gathered cluster points) land in page-locked blocks the CALLING THREAD keeps between calls: the
// kernels store into them directly and the next call of the same size pins nothing.  Retention is bounded: a block
// is given back when a request needs less than a quarter of it, a thread keeps at most kHostScratchBudget bytes, and
// ReleaseHostScratch() frees the calling thread's blocks at once (a long-lived host calls it after its last big cloud).
namespace detail {
constexpr size_t kHostScratchBudget = (size_t)1 << 30;   // 1 GiB of page-locked memory per thread, at most
struct PinnedScratch {
    void* p = nullptr;
    size_t cap = 0;
    void release() {
        if (p) m3d_host_free(p);
        p = nullptr;
        cap = 0;
    }
    // nullptr: over the budget or the allocation failed -- the caller falls back to pageable memory
    void* get(size_t bytes) {
        if (bytes > kHostScratchBudget) {
            release();
            return nullptr;
        }
        if (bytes > cap || (cap > ((size_t)64 << 20) && bytes < cap / 4)) {
            release();
            p = m3d_host_alloc(bytes);
            cap = p ? bytes : 0;
        }
        return p;
    }
    // (no destructor: a thread-local of the main thread dies at process exit, possibly after the HIP runtime)
};
inline PinnedScratch& host_scratch(int which) {   // 0: index lists, 1: gathered points
    static thread_local PinnedScratch s[2];
    return s[which & 1];
}
}  // namespace detail
namespace detail {
// the rows of level l after an m3d_voxel_down_sample* call that wrote m of them into clouds sized for n
inline void voxel_shrink(PointCloud& pc, size_t m, bool nrm, bool col) {
    pc.points_.resize(m);
    pc.normals_.resize(nrm ? m : 0);
    pc.colors_.resize(col ? m : 0);
}
}  // namespace detail

inline PointCloud PointCloud::VoxelDownSample(double voxel_size, int device) const {
    const size_t n = points_.size();
    const bool nrm = HasNormals(), col = HasColors();
    PointCloud out;
    out.points_.resize(n);
    if (nrm) out.normals_.resize(n);
    if (col) out.colors_.resize(n);
    size_t m = 0;
    const int rc = m3d_voxel_down_sample(n ? points_[0].data() : nullptr, nrm ? normals_[0].data() : nullptr,
                                         col ? colors_[0].data() : nullptr, n, voxel_size, device,
                                         n ? out.points_[0].data() : nullptr, nrm ? out.normals_[0].data() : nullptr,
                                         col ? out.colors_[0].data() : nullptr, nullptr, nullptr, &m, nullptr);
    if (rc < 0) throw std::runtime_error(std::string("[Misc3D Error] ") + m3d_last_error());   // (logging.h's LogError)
    detail::voxel_shrink(out, m, nrm, col);
    return out;
}

inline void ReleaseHostScratch() {
    detail::host_scratch(0).release();
    detail::host_scratch(1).release();
}

}  // namespace misc3d
