// misc3d/common/knn.h -- host mirror of the reference's include/misc3d/common/knn.h (KNearestSearch, src/knn.cpp) over
// the C ABI (m3d_knn_*).  Header-only; no Eigen / Open3D / Annoy needed.
//
// The reference answers with an Annoy index (approximate); this class returns the exact answer Annoy approximates, in the
// order and with the quirks written down next to m3d_knn_search in include/misc3d_amd.h.  Data is dim x N column-major
// (Eigen::MatrixXd, open3d Feature::data_): N contiguous rows of dim doubles.  n_trees is kept and has no effect.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <vector>

#include <misc3d/features/boundary_detection.h>
#include <misc3d/geometry.h>
#include <misc3d/logging.h>
#include <misc3d/registration/correspondence_matching.h>
#include <misc3d_amd.h>

namespace misc3d {
namespace common {

/**
 * @brief Exact K nearest neighbour search over the columns of a dim x N matrix, on the device.
 */
class KNearestSearch {
public:
    KNearestSearch() : n_trees_(4) {}
    explicit KNearestSearch(int n_trees) : n_trees_(n_trees) {}
    KNearestSearch(const double* data, size_t rows, size_t cols, int n_trees = 4) : n_trees_(n_trees) {
        SetMatrixData(data, rows, cols);
    }
    KNearestSearch(const CloudView& geometry, int n_trees = 4) : n_trees_(n_trees) { SetGeometry(geometry); }
    KNearestSearch(const registration::FeatureView& feature, int n_trees = 4) : n_trees_(n_trees) { SetFeature(feature); }
    ~KNearestSearch() { Reset(); }
    KNearestSearch(const KNearestSearch&) = delete;
    KNearestSearch& operator=(const KNearestSearch&) = delete;

    /** The device of the next Set* (default 0). */
    void SetDevice(int device) { device_ = device; }
    int GetTrees() const { return n_trees_; }
    size_t Size() const { return index_ ? m3d_knn_size(index_) : 0; }
    size_t Dimension() const { return dimension_; }

    /** data: rows x cols column-major (rows = dimension, cols = points).  0 rows or 0 columns: false, the index empty. */
    bool SetMatrixData(const double* data, size_t rows, size_t cols) {
        Reset();
        dimension_ = rows;
        if (rows == 0 || cols == 0) return false;
        if (rows > 1024) LogError("KNearestSearch: dimension " + std::to_string(rows) + " above 1024");
        index_ = m3d_knn_create(data, cols, (int)rows, device_, nullptr);
        if (!index_) LogError(m3d_last_error());
        return true;
    }
    bool SetGeometry(const CloudView& geometry) { return SetMatrixData(geometry.xyz, 3, geometry.n); }
    bool SetGeometry(const PointCloud& geometry) { return SetGeometry(CloudView(geometry)); }
    bool SetFeature(const registration::FeatureView& feature) {
        return SetMatrixData(feature.data, (size_t)feature.dim, feature.n);
    }

    int Search(const std::vector<double>& query, const features::KDTreeSearchParamKNN& param, std::vector<size_t>& indices,
               std::vector<double>& distance) const {
        return SearchKNN(query, param.knn_, indices, distance);
    }
    int Search(const std::vector<double>& query, const features::KDTreeSearchParamHybrid& param,
               std::vector<size_t>& indices, std::vector<double>& distance) const {
        return SearchHybrid(query, param.radius_, param.max_nn_, indices, distance);
    }
    /** Radius search is not supported (knn.cpp:97-99): -1. */
    int Search(const std::vector<double>&, const features::KDTreeSearchParamRadius&, std::vector<size_t>&,
               std::vector<double>&) const {
        return -1;
    }

    /** knn.cpp:103-113: -1 for an empty index, query.size() != dimension or knn < 0; else the number of results. */
    int SearchKNN(const std::vector<double>& query, int knn, std::vector<size_t>& indices, std::vector<double>& distance) const {
        if (!index_ || query.size() != dimension_ || knn < 0) return -1;
        std::vector<int64_t> counts;
        Run(query.data(), 1, M3D_KNN_SEARCH_KNN, knn, 0.0, indices, distance, counts, true);
        return (int)counts[0];
    }
    /** knn.cpp:115-139, quirks included: the last in-radius neighbour is dropped, and when even the nearest one is
     * beyond the radius (or knn == 0) the reference's resize(SIZE_MAX) throws std::length_error -- so does this. */
    int SearchHybrid(const std::vector<double>& query, double radius, int knn, std::vector<size_t>& indices,
                     std::vector<double>& distance) const {
        if (!index_ || query.size() != dimension_ || knn < 0) return -1;
        std::vector<int64_t> counts;
        Run(query.data(), 1, M3D_KNN_SEARCH_HYBRID, knn, radius, indices, distance, counts, true);
        if (counts[0] < 0) throw std::length_error("vector::_M_default_append");
        return (int)counts[0];
    }

    /** Batch form: m queries (row-major m x dimension).  indices / distance: m x kout row-major, kout = min(knn, N), padded
     * with SIZE_MAX / +inf past counts[q]; counts[q] = the single form's return value, -1 where SearchHybrid throws.
     * Returns kout, or -1 where the single form returns -1. */
    int SearchKNNBatch(const double* queries, size_t m, int knn, std::vector<size_t>& indices, std::vector<double>& distance,
                       std::vector<int64_t>& counts) const {
        if (!index_ || knn < 0) return -1;
        return Run(queries, m, M3D_KNN_SEARCH_KNN, knn, 0.0, indices, distance, counts);
    }
    int SearchHybridBatch(const double* queries, size_t m, double radius, int knn, std::vector<size_t>& indices,
                          std::vector<double>& distance, std::vector<int64_t>& counts) const {
        if (!index_ || knn < 0) return -1;
        return Run(queries, m, M3D_KNN_SEARCH_HYBRID, knn, radius, indices, distance, counts);
    }

private:
    void Reset() {
        if (index_) m3d_knn_destroy(index_);
        index_ = nullptr;
        dimension_ = 0;
    }
    // m queries -> row-major m x kout outputs; the single-query forms trim their row to counts[0]
    int Run(const double* queries, size_t m, int search, int knn, double radius, std::vector<size_t>& indices,
            std::vector<double>& distance, std::vector<int64_t>& counts, bool single = false) const {
        const size_t kout = std::min<size_t>((size_t)knn, m3d_knn_size(index_));
        indices.assign(m * kout, 0);
        distance.assign(m * kout, 0.0);
        counts.assign(m, 0);
        CheckStatus(m3d_knn_search(index_, queries, m, search, knn, radius, kout, indices.data(), distance.data(), nullptr,
                                   counts.data(), nullptr));
        if (single) {
            const size_t keep = counts[0] > 0 ? (size_t)counts[0] : 0;
            indices.resize(keep);
            distance.resize(keep);
        }
        return (int)kout;
    }

    int n_trees_;
    int device_ = 0;
    size_t dimension_ = 0;
    m3d_knn* index_ = nullptr;
};

}  // namespace common
}  // namespace misc3d
