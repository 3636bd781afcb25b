// misc3d/segmentation/proximity_extraction.h -- host mirror of the reference's
// include/misc3d/segmentation/proximity_extraction.h (ProximityExtractor and its evaluators, src/proximity_extraction.cpp)
// over the C ABI.  Header-only; no Eigen / Open3D needed.
//
// The built-in evaluators describe themselves (Describe) and run on the device (m3d_proximity_segment / _nn).  Any other
// subclass of BaseProximityEvaluator runs on the host: the device builds the radius neighbour lists
// (m3d_radius_neighbors), the host unites every pair that the evaluator accepts in either direction.  That path calls the
// evaluator once or twice per neighbour pair and is slow by nature.
//
// Output order: clusters by size descending, ties by their smallest point index ascending (the reference's unstable
// std::sort leaves it open); indices within a cluster ascending.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <numeric>
#include <algorithm>
#include <vector>

#include <misc3d/geometry.h>
#include <misc3d/logging.h>
#include <misc3d_amd.h>

namespace misc3d {
namespace segmentation {

/**
 * @brief Base Proximity Evaluation class: operator()(i, j, dist) decides whether neighbours i and j belong together.
 */
class BaseProximityEvaluator {
public:
    virtual ~BaseProximityEvaluator() = default;
    virtual bool operator()(size_t i, size_t j, double dist) const = 0;
    // the device form of a built-in evaluator: false for any other subclass (host path)
    virtual bool Describe(m3d_proximity_evaluator* ev, const double** normals, size_t* n_normals) const { return false; }
};

namespace detail {
inline bool NormalsAccept(const std::vector<Vector3d>& normals, double max_angle, size_t i, size_t j) {
    if (i >= normals.size() || j >= normals.size()) LogError("Index exceed size of data!");
    const Vector3d& a = normals[i];
    const Vector3d& b = normals[j];
    const double angle = std::acos((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]);
    if (max_angle >= 0.0) return angle <= max_angle;
    return std::min(angle, M_PI - angle) <= -max_angle;
}
inline double Deg2Rad(double angle_deg) { return angle_deg / 180 * M_PI; }
}  // namespace detail

class DistanceProximityEvaluator : public BaseProximityEvaluator {
public:
    DistanceProximityEvaluator(double dist_thresh) : max_distance_(dist_thresh) {}
    bool operator()(size_t, size_t, double dist) const override { return dist < max_distance_; }
    bool Describe(m3d_proximity_evaluator* ev, const double** normals, size_t* n_normals) const override {
        *ev = m3d_proximity_evaluator{M3D_PROX_DISTANCE, 0, max_distance_, 0.0};
        *normals = nullptr;
        *n_normals = 0;
        return true;
    }

private:
    double max_distance_;
};

class NormalsProximityEvaluator : public BaseProximityEvaluator {
public:
    /** @param angle_thresh angle in degrees (negative: unoriented normals, the angle or its supplement) */
    NormalsProximityEvaluator(const std::vector<Vector3d>& normals, double angle_thresh)
        : normals_(normals), angle_deg_(angle_thresh), max_angle_(detail::Deg2Rad(angle_thresh)) {}
    bool operator()(size_t i, size_t j, double) const override {
        return detail::NormalsAccept(normals_, max_angle_, i, j);
    }
    bool Describe(m3d_proximity_evaluator* ev, const double** normals, size_t* n_normals) const override {
        *ev = m3d_proximity_evaluator{M3D_PROX_NORMALS, 0, 0.0, angle_deg_};
        *normals = normals_.empty() ? nullptr : normals_[0].data();
        *n_normals = normals_.size();
        return true;
    }

private:
    std::vector<Vector3d> normals_;
    double angle_deg_, max_angle_;
};

class DistanceNormalsProximityEvaluator : public BaseProximityEvaluator {
public:
    DistanceNormalsProximityEvaluator(const std::vector<Vector3d>& normals, double dist_thresh, double angle_thresh)
        : normals_(normals), max_distance_(dist_thresh), angle_deg_(angle_thresh),
          max_angle_(detail::Deg2Rad(angle_thresh)) {}
    bool operator()(size_t i, size_t j, double dist) const override {
        if (i >= normals_.size() || j >= normals_.size()) LogError("Index exceed size of data!");
        if (dist >= max_distance_) return false;
        return detail::NormalsAccept(normals_, max_angle_, i, j);
    }
    bool Describe(m3d_proximity_evaluator* ev, const double** normals, size_t* n_normals) const override {
        *ev = m3d_proximity_evaluator{M3D_PROX_DISTANCE_NORMALS, 0, max_distance_, angle_deg_};
        *normals = normals_.empty() ? nullptr : normals_[0].data();
        *n_normals = normals_.size();
        return true;
    }

private:
    std::vector<Vector3d> normals_;
    double max_distance_, angle_deg_, max_angle_;
};

class ProximityExtractor {
public:
    ProximityExtractor() : ProximityExtractor(1) {}
    ProximityExtractor(size_t min_cluster_size)
        : ProximityExtractor(min_cluster_size, std::numeric_limits<size_t>::max()) {}
    ProximityExtractor(size_t min_cluster_size, size_t max_cluster_size)
        : min_cluster_size_(min_cluster_size), max_cluster_size_(max_cluster_size) {}

    void SetDevice(int device) { device_ = device; }

    /**
     * @brief Segment a point cloud given the radius of the neighbour search.
     */
    std::vector<std::vector<size_t>> Segment(const CloudView& pc, double search_radius,
                                             const BaseProximityEvaluator& evaluator) {
        m3d_proximity_evaluator ev;
        const double* normals = nullptr;
        size_t n_normals = 0;
        Begin(pc.n);
        if (evaluator.Describe(&ev, &normals, &n_normals)) {
            size_t k = 0;
            CheckStatus(m3d_proximity_segment(pc.xyz, normals, n_normals, pc.n, search_radius, &ev, min_cluster_size_,
                                              max_cluster_size_, device_, offsets_.data(), indices_.data(), &k, nullptr,
                                              nullptr));
            return Finish(k);
        }
        // host path: device-built neighbour lists, the evaluator asked for every ordered pair whose ends are still apart
        std::vector<size_t> off(pc.n + 1);
        size_t total = 0;
        CheckStatus(m3d_radius_neighbors(pc.xyz, pc.n, search_radius, device_, off.data(), nullptr, nullptr, 0, &total));
        std::vector<uint32_t> nb(std::max<size_t>(total, 1));
        std::vector<double> d2(std::max<size_t>(total, 1));
        CheckStatus(m3d_radius_neighbors(pc.xyz, pc.n, search_radius, device_, off.data(), nb.data(), d2.data(), total,
                                         &total));
        std::vector<size_t> parent(pc.n);
        std::iota(parent.begin(), parent.end(), (size_t)0);
        for (size_t i = 0; i < pc.n; ++i)
            for (size_t k = off[i]; k < off[i + 1]; ++k)
                if (Find(parent, i) != Find(parent, nb[k]) && evaluator(i, nb[k], std::sqrt(d2[k]))) Unite(parent, i, nb[k]);
        return Order(parent);
    }

    /**
     * @brief Segment a point cloud given the neighbour lists of its points (entry 0 of every list is skipped, as the
     * reference skips the query itself).
     */
    std::vector<std::vector<size_t>> Segment(const CloudView& pc, const std::vector<std::vector<size_t>>& nn_indices,
                                             const BaseProximityEvaluator& evaluator) {
        if (pc.n != nn_indices.size()) LogError("The number of input data size are not equal!");
        m3d_proximity_evaluator ev;
        const double* normals = nullptr;
        size_t n_normals = 0;
        Begin(pc.n);
        if (evaluator.Describe(&ev, &normals, &n_normals)) {
            std::vector<size_t> off(pc.n + 1, 0), idx;
            for (size_t i = 0; i < pc.n; ++i) off[i + 1] = off[i] + nn_indices[i].size();
            idx.reserve(off[pc.n]);
            for (const auto& l : nn_indices) idx.insert(idx.end(), l.begin(), l.end());
            size_t k = 0;
            CheckStatus(m3d_proximity_segment_nn(pc.xyz, normals, n_normals, pc.n, nn_indices.size(), off.data(),
                                                 idx.empty() ? nullptr : idx.data(), &ev, min_cluster_size_,
                                                 max_cluster_size_, device_, offsets_.data(), indices_.data(), &k,
                                                 nullptr, nullptr));
            return Finish(k);
        }
        std::vector<size_t> parent(pc.n);
        std::iota(parent.begin(), parent.end(), (size_t)0);
        for (size_t i = 0; i < pc.n; ++i)
            for (size_t k = 1; k < nn_indices[i].size(); ++k) {
                const size_t j = nn_indices[i][k];
                if (j >= pc.n) LogError("neighbour index outside the cloud");
                const double dx = pc.xyz[3 * i] - pc.xyz[3 * j], dy = pc.xyz[3 * i + 1] - pc.xyz[3 * j + 1],
                             dz = pc.xyz[3 * i + 2] - pc.xyz[3 * j + 2];
                if (Find(parent, i) != Find(parent, j) && evaluator(i, j, std::sqrt((dx * dx + dy * dy) + dz * dz)))
                    Unite(parent, i, j);
            }
        return Order(parent);
    }

    /**
     * @brief Cluster id of every point of the last Segment; points of no cluster get GetClusterNum().  Like the
     * reference, the map is a member that is only resized: entries of an earlier, larger cloud stay where no cluster of
     * the last call overwrites them.
     */
    std::vector<size_t> GetClusterIndexMap() {
        indices_map_.resize(points_num_, cluster_num_);
        for (size_t c = 0; c < clustered_indices_map_.size(); ++c)
            for (size_t i : clustered_indices_map_[c]) indices_map_[i] = c;
        return indices_map_;
    }
    size_t GetClusterNum() { return cluster_num_; }

private:
    static size_t Find(std::vector<size_t>& parent, size_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    }
    static void Unite(std::vector<size_t>& parent, size_t a, size_t b) {
        a = Find(parent, a);
        b = Find(parent, b);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);   // the root stays the smallest index
    }
    void Begin(size_t n) {
        points_num_ = n;
        offsets_.assign(n + 1, 0);
        indices_.assign(std::max<size_t>(n, 1), 0);
    }
    std::vector<std::vector<size_t>> Finish(size_t k) {
        std::vector<std::vector<size_t>> out(k);
        for (size_t c = 0; c < k; ++c) out[c].assign(indices_.begin() + offsets_[c], indices_.begin() + offsets_[c + 1]);
        return Keep(std::move(out));
    }
    std::vector<std::vector<size_t>> Order(std::vector<size_t>& parent) {
        const size_t n = parent.size();
        std::vector<size_t> size(n, 0), root(n);
        for (size_t i = 0; i < n; ++i) ++size[root[i] = Find(parent, i)];
        std::vector<size_t> kept;
        for (size_t r = 0; r < n; ++r)
            if (root[r] == r && size[r] >= min_cluster_size_ && size[r] <= max_cluster_size_) kept.push_back(r);
        std::stable_sort(kept.begin(), kept.end(), [&](size_t a, size_t b) { return size[a] > size[b]; });
        std::vector<size_t> rank(n, SIZE_MAX);
        for (size_t k = 0; k < kept.size(); ++k) rank[kept[k]] = k;
        std::vector<std::vector<size_t>> out(kept.size());
        for (size_t i = 0; i < n; ++i)
            if (rank[root[i]] != SIZE_MAX) out[rank[root[i]]].push_back(i);
        return Keep(std::move(out));
    }
    std::vector<std::vector<size_t>> Keep(std::vector<std::vector<size_t>> out) {
        clustered_indices_map_ = out;
        cluster_num_ = out.size();
        return out;
    }

    size_t min_cluster_size_, max_cluster_size_;
    size_t cluster_num_ = 0, points_num_ = 0;
    int device_ = 0;
    std::vector<size_t> offsets_, indices_, indices_map_;
    std::vector<std::vector<size_t>> clustered_indices_map_;
};

}  // namespace segmentation
}  // namespace misc3d
