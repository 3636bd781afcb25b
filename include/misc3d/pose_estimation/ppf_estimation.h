// misc3d/pose_estimation/ppf_estimation.h -- the reference's PPFEstimator and PPFEstimatorConfig
// (include/misc3d/pose_estimation/ppf_estimation.h, src/ppf_estimation.cpp) as a host mirror over the C ABI: Train is
// m3d_ppf_prepare_model (PreprocessTrain; the contract "PPF model preprocessing" of include/misc3d_amd.h) and a PPFVoting of
// its sample, Estimate is m3d_ppf_prepare_scene, m3d_ppf_reference_indices and PPFVoting's Estimate.  Header-only; no Eigen /
// Open3D needed.
//
// Errors follow the convention of misc3d/logging.h, which is the reference's: LogError THROWS std::runtime_error with the
// reference's message (the `return false` the reference writes behind it is never reached there either).  Train returns false
// only where PPFVoting refuses the sample's size.
//
// Departures from the reference, all stated in include/misc3d_amd.h and DESIGN.md: the model's box is rule B1's PCA box of all
// points, not Qhull's hull (Train takes the reference's box when the caller has it); dist_threshold = rel_dist_thresh x
// diameter is computed afresh by every Train (the reference multiplies its member again on each call); Estimate takes the seed
// of the reference points' std::mt19937 (the reference draws it from std::random_device).
#pragma once
#include <array>
#include <cstdint>
#include <random>
#include <vector>

#include <misc3d/geometry.h>
#include <misc3d/logging.h>
#include <misc3d/pose_estimation/ppf_voting.h>
#include <misc3d_amd.h>

namespace misc3d {
namespace pose_estimation {

/** The reference's config: fields, nesting, defaults (src/ppf_estimation.cpp:1392-1405) and enum names; angles in radians. */
class PPFEstimatorConfig {
public:
    enum class ReferencePointSelection { Random };
    using RefineMethod = misc3d::pose_estimation::RefineMethod;
    enum class VotingMode { SampledPoints, EdgePoints };

    struct TrainingParam {
        bool invert_model_normal = false;
        bool use_external_normal = false;
        double rel_sample_dist = 0.05;
        double rel_dense_sample_dist = 0.025;
        double calc_normal_relative = 0.01;
    };
    struct ReferenceParam {
        ReferencePointSelection method = ReferencePointSelection::Random;
        double ratio = 0.6;
    };
    struct VotingParam {
        VotingMode method = VotingMode::SampledPoints;
        bool faster_mode = true;
        double angle_step = 12.0 / 180.0 * 3.14159265358979323846;
        double min_dist_thresh = 1.0 / 3;
        double min_angle_thresh = 30.0 / 180.0 * 3.14159265358979323846;
    };
    struct EdgeParam {
        size_t pts_num = 20;
    };
    struct RefineParam {
        RefineMethod method = RefineMethod::PointToPlane;
        double rel_dist_sparse_thresh = 5;
    };

    TrainingParam training_param_;
    ReferenceParam ref_param_;
    VotingParam voting_param_;
    EdgeParam edge_param_;
    RefineParam refine_param_;
    double rel_dist_thresh_ = 0.05;
    double rel_angle_thresh_ = 12.0 / 180.0 * 3.14159265358979323846;
    double score_thresh_ = 0.6;
    size_t num_result_ = 10;
    size_t object_id_ = 0;
};

class PPFEstimator {
public:
    PPFEstimator() = default;
    explicit PPFEstimator(const PPFEstimatorConfig& config, int device = 0) : device_(device) { SetConfig(config); }

    /** CheckConfig (:1409-1418) */
    static bool CheckConfig(const PPFEstimatorConfig& config) {
        if (config.training_param_.rel_dense_sample_dist >= config.training_param_.rel_sample_dist) {
            LogError("Dense_sample_dist should be smaller than sample_dist.");
            return false;
        }
        return true;
    }
    bool SetConfig(const PPFEstimatorConfig& config) {
        if (!CheckConfig(config)) return false;
        config_ = config;
        return true;
    }

    /** Train (:526-601).  box_center / box_extent (3 doubles each, both or neither): the reference's oriented bounding box. */
    bool Train(const CloudView& pc, const double* box_center = nullptr, const double* box_extent = nullptr) {
        Clear();
        if (pc.n == 0) {
            LogError("There is no input points");
            return false;
        }
        const bool edge = EdgeMode();
        m3d_ppf_train_params tp;
        m3d_ppf_train_params_default_(&tp);
        tp.rel_sample_dist = config_.training_param_.rel_sample_dist;
        tp.rel_dense_sample_dist = edge ? config_.training_param_.rel_dense_sample_dist : 0.0;
        tp.calc_normal_relative = config_.training_param_.calc_normal_relative;
        tp.invert_model_normal = config_.training_param_.invert_model_normal;
        tp.use_external_normal = config_.training_param_.use_external_normal;
        tp.pts_num = static_cast<int32_t>(config_.edge_param_.pts_num);
        std::vector<double> normals(3 * pc.n);
        std::vector<size_t> si(pc.n), di(edge ? pc.n : 0), ei(edge ? pc.n : 0);
        size_t ns = 0, nd = 0, ne = 0;
        CheckStatus(m3d_ppf_prepare_model(pc.xyz, pc.normals, pc.n, &tp, box_center, box_extent, device_, normals.data(), si.data(), &ns,
                                          edge ? di.data() : nullptr, &nd, edge ? ei.data() : nullptr, &ne, &info_));
        if (ns == 0) {
            LogError("There is no input points after preprocessing");
            return false;
        }
        auto gather = [&](const std::vector<size_t>& idx, size_t k, PointCloud* out) {
            out->points_.resize(k);
            out->normals_.resize(k);
            for (size_t j = 0; j < k; ++j)
                for (int a = 0; a < 3; ++a) {
                    out->points_[j][a] = pc.xyz[3 * idx[j] + a];
                    out->normals_[j][a] = normals[3 * idx[j] + a];
                }
        };
        gather(si, ns, &model_sample_);
        m3d_ppf_params vp = PPFVoting::DefaultParams();
        vp.rel_sample_dist = config_.training_param_.rel_sample_dist;
        vp.angle_step = config_.voting_param_.angle_step;
        vp.min_dist_thresh = config_.voting_param_.min_dist_thresh;
        vp.min_angle_thresh = config_.voting_param_.min_angle_thresh;
        vp.faster_mode = config_.voting_param_.faster_mode;
        try {
            if (edge) {
                if (ne == 0) {
                    LogError("Fail to extract edge points!");
                    return false;
                }
                std::vector<size_t> into_model(ne);
                for (size_t j = 0; j < ne; ++j) into_model[j] = di[ei[j]];
                gather(into_model, ne, &model_edges_);
                voting_.TrainEdges(model_sample_.points_[0].data(), model_sample_.normals_[0].data(), ns, model_edges_.points_[0].data(),
                                   model_edges_.normals_[0].data(), ne, info_.diameter, info_.r_min, vp, device_);
            } else {
                voting_.Train(model_sample_.points_[0].data(), model_sample_.normals_[0].data(), ns, info_.diameter, info_.r_min, vp, device_);
            }
        } catch (const std::runtime_error& e) {
            // the sample exceeds what PPFVoting accepts (m3d_ppf_model_create's size refusals): false; anything else goes on up
            const std::string what = e.what();
            if (what.find("ppf: the model must have") == std::string::npos && what.find("ppf: the table's sort scratch") == std::string::npos) throw;
            LogWarning(what);
            return false;
        }
        dist_threshold_ = config_.rel_dist_thresh_ * info_.diameter;
        trained_ = true;
        return true;
    }

    /** Estimate (:280-397).  seed: of the reference points' std::mt19937; null: drawn from std::random_device. */
    bool Estimate(const CloudView& pc, std::vector<Pose6D>& results, const uint32_t* seed = nullptr) {
        results.clear();
        pose_list_.clear();
        if (!trained_) {
            LogError("Need training before estimating!");
            return false;
        }
        const bool edge = EdgeMode();
        PreparedScene s = PPFVoting::PrepareScene(pc.xyz, pc.normals, pc.n, info_.diameter, config_.training_param_.calc_normal_relative,
                                                  info_.dist_step, edge ? info_.dist_step_dense : 0.0,
                                                  static_cast<int>(config_.edge_param_.pts_num), device_);
        const size_t num = s.sample_points.size() / 3;
        Fill(s.sample_points, s.sample_normals, &scene_sample_);
        if (num == 0) return false;
        std::vector<double> ep, en;
        if (edge) {
            if (s.edge_indices.empty()) return false;
            for (size_t i : s.edge_indices)
                for (int a = 0; a < 3; ++a) {
                    ep.push_back(s.dense_points[3 * i + a]);
                    en.push_back(s.dense_normals[3 * i + a]);
                }
            Fill(ep, en, &scene_edges_);
        }
        std::vector<size_t> reference(static_cast<size_t>(config_.ref_param_.ratio * num));
        CheckStatus(m3d_ppf_reference_indices(num, reference.size(), seed ? *seed : std::random_device{}(), reference.data()));
        const PPFClusterParams cp{dist_threshold_, config_.rel_angle_thresh_, config_.ref_param_.ratio, config_.score_thresh_,
                                  config_.refine_param_.rel_dist_sparse_thresh, static_cast<int>(config_.num_result_),
                                  config_.refine_param_.method, static_cast<int>(config_.object_id_)};
        results = edge ? voting_.EstimateEdges(s.sample_points.data(), s.sample_normals.data(), num, reference, ep.data(), en.data(),
                                               ep.size() / 3, cp)
                       : voting_.Estimate(s.sample_points.data(), s.sample_normals.data(), num, reference, cp);
        pose_list_ = results;
        return !results.empty();
    }

    double GetModelDiameter() const { return info_.diameter; }
    std::vector<Pose6D> GetPose() const { return pose_list_; }
    PointCloud GetSampledModel() const { return model_sample_; }
    PointCloud GetSampledScene() const { return scene_sample_; }
    PointCloud GetModelEdges() const { return Edges(model_edges_, "model"); }
    PointCloud GetSceneEdges() const { return Edges(scene_edges_, "scene"); }
    /** what PreprocessTrain derived (B1, B2, the seed, the orientation's stats) */
    const m3d_ppf_model_info& GetModelInfo() const { return info_; }
    double GetDistThreshold() const { return dist_threshold_; }

private:
    bool EdgeMode() const { return config_.voting_param_.method == PPFEstimatorConfig::VotingMode::EdgePoints; }
    static void Fill(const std::vector<double>& p, const std::vector<double>& n, PointCloud* out) {
        out->points_.resize(p.size() / 3);
        out->normals_.resize(p.size() / 3);
        for (size_t k = 0; k < p.size(); ++k) {
            out->points_[k / 3][k % 3] = p[k];
            out->normals_[k / 3][k % 3] = n[k];
        }
    }
    PointCloud Edges(const PointCloud& pc, const char* what) const {
        if (!EdgeMode()) LogWarning(std::string("Can not get ") + what + " edge points due to edge support is not enabled.");
        return pc;
    }
    void Clear() {
        trained_ = false;
        info_ = m3d_ppf_model_info{};
        dist_threshold_ = 0.0;
        model_sample_ = model_edges_ = scene_sample_ = scene_edges_ = PointCloud();
        pose_list_.clear();
    }

    PPFEstimatorConfig config_;
    int device_ = 0;
    bool trained_ = false;
    m3d_ppf_model_info info_{};
    double dist_threshold_ = 0.0;
    PPFVoting voting_;
    PointCloud model_sample_, model_edges_, scene_sample_, scene_edges_;
    std::vector<Pose6D> pose_list_;
};

}  // namespace pose_estimation
}  // namespace misc3d
