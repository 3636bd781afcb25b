// misc3d/pose_estimation/ppf_voting.h -- host mirror over the C ABI (m3d_ppf_*) of the device hot paths of the reference's
// PPFEstimator (src/ppf_estimation.cpp): the point-pair table of a model (CalcHashTable, :603-640), the vote of a scene
// against it (VotingAndGetPose, :399-524), and the way from the raw poses to ranked, refined results (ClusterPoses,
// PoseAverage, RefineSparsePose, the centre shift and the scoring).  Header-only; no Eigen / Open3D needed.
//
// All take ALREADY SAMPLED points with unit normals, in either voting mode: Train / Vote / Estimate are SampledPoints,
// TrainEdges / VoteEdges / EstimateEdges are EdgePoints; PrepareScene is PreprocessEstimate.  PreprocessTrain and the
// PPFEstimator / PPFEstimatorConfig classes are in ppf_estimation.h beside this header; the contract of what is here is written down
// next to m3d_ppf_vote, m3d_ppf_vote_edges and m3d_ppf_estimate in include/misc3d_amd.h.
#pragma once
#include <array>
#include <cstdint>
#include <vector>

#include <misc3d/geometry.h>
#include <misc3d/logging.h>
#include <misc3d_amd.h>

namespace misc3d {
namespace pose_estimation {

/** One raw pose of the reference's pose_list (Pose6D: pose_, num_votes_, corr_mi_), for the CENTRED model. */
struct VotedPose {
    std::array<double, 16> pose;   // row-major 4 x 4
    size_t num_votes;
    size_t corr_mi;                // model index
    size_t reference;              // position in the reference index list the pose was voted at
    size_t alpha_index;
};

/** The reference's Pose6D (data_structure.h): a result of Estimate, for the UNCENTRED model. */
struct Pose6D {
    std::array<double, 16> pose;   // row-major 4 x 4
    std::array<double, 4> q;       // w, x, y, z
    std::array<double, 3> t;
    size_t num_votes;
    double score;
    int object_id;
};

/** PPFEstimatorConfig::RefineMethod */
enum class RefineMethod { NoRefine = M3D_PPF_REFINE_NONE, PointToPoint = M3D_PPF_REFINE_POINT_TO_POINT, PointToPlane = M3D_PPF_REFINE_POINT_TO_PLANE };

/** m3d_ppf_cluster_params with the method as the reference's enum. */
struct PPFClusterParams {
    double dist_threshold, angle_threshold, ratio, score_thresh, rel_dist_sparse_thresh;
    int num_result;
    RefineMethod refine_method;
    int object_id;
    m3d_ppf_cluster_params c() const {
        return m3d_ppf_cluster_params{dist_threshold, angle_threshold, ratio, score_thresh, rel_dist_sparse_thresh, num_result,
                                      static_cast<int32_t>(refine_method), object_id, 0};
    }
};

/** What ClusterPoses returns: per valid pose (votes descending, ties by input index), per translation cluster, per sub-cluster. */
struct PoseClusters {
    std::vector<uint32_t> order, count_t, count_r;
    std::vector<int32_t> label_t, label_r;
    int32_t min_num_pt_t = 0;
    std::vector<int32_t> min_num_pt_r;
    std::vector<uint64_t> cluster_votes;
    std::vector<std::array<double, 16>> avg_poses;
    std::vector<uint64_t> avg_votes;
    std::vector<uint32_t> avg_cluster;
    m3d_ppf_cluster_stats stats{};
};

/** What PreprocessEstimate leaves (m3d_ppf_prepare_scene): the sample, the dense sample and the dense sample's edge points. */
struct PreparedScene {
    std::vector<double> sample_points, sample_normals;   // row-major k x 3 each
    std::vector<double> dense_points, dense_normals;     // empty without the edge part
    std::vector<size_t> edge_indices;                    // ascending, into the dense sample
};

class PPFVoting {
public:
    /** The reference's defaults (angles in radians). */
    static m3d_ppf_params DefaultParams() {
        m3d_ppf_params p;
        m3d_ppf_default_params(&p);
        return p;
    }

    PPFVoting() = default;
    ~PPFVoting() { Reset(); }
    PPFVoting(const PPFVoting&) = delete;
    PPFVoting& operator=(const PPFVoting&) = delete;

    /** Train (:537-570) on n sampled points with unit normals (row-major n x 3 each). */
    void Train(const double* points, const double* normals, size_t n, double diameter, double r_min,
               const m3d_ppf_params& params = DefaultParams(), int device = 0) {
        Reset();
        model_ = m3d_ppf_model_create(points, normals, n, diameter, r_min, &params, device, nullptr);
        if (!model_) LogError(m3d_last_error());
    }
    /** Train with edge support (:572-593, VotingMode::EdgePoints): the table pairs the n sample points with the n_edge edge points. */
    void TrainEdges(const double* points, const double* normals, size_t n, const double* edge_points, const double* edge_normals,
                    size_t n_edge, double diameter, double r_min, const m3d_ppf_params& params = DefaultParams(), int device = 0) {
        Reset();
        model_ = m3d_ppf_model_create_edges(points, normals, n, edge_points, edge_normals, n_edge, diameter, r_min, &params, device, nullptr);
        if (!model_) LogError(m3d_last_error());
    }
    bool IsTrained() const { return model_ != nullptr; }
    size_t Size() const { return m3d_ppf_model_size(model_); }
    /** The model's edge points; 0 for a SampledPoints model. */
    size_t EdgeSize() const { return m3d_ppf_model_edge_size(model_); }
    bool IsEdgeMode() const { return EdgeSize() != 0; }
    std::array<double, 3> Centroid() const {
        std::array<double, 3> c{0, 0, 0};
        if (model_) CheckStatus(m3d_ppf_model_centroid(model_, c.data()));
        return c;
    }
    /** The opaque model, for m3d_ppf_model_table. */
    const m3d_ppf_model* Handle() const { return model_; }

    /** VotingAndGetPose: the raw poses in ascending (reference position, model index). */
    std::vector<VotedPose> Vote(const double* scene_points, const double* scene_normals, size_t m,
                                const std::vector<size_t>& reference, m3d_ppf_vote_stats* stats = nullptr) const {
        return VoteImpl(scene_points, scene_normals, m, reference, nullptr, nullptr, 0, false, stats);
    }

    /** VotingAndGetPose of an EdgePoints model (:319-328): reference points from the scene sample, neighbours from the scene's edges. */
    std::vector<VotedPose> VoteEdges(const double* scene_points, const double* scene_normals, size_t m, const std::vector<size_t>& reference,
                                     const double* scene_edge_points, const double* scene_edge_normals, size_t m_edge,
                                     m3d_ppf_vote_stats* stats = nullptr) const {
        return VoteImpl(scene_points, scene_normals, m, reference, scene_edge_points, scene_edge_normals, m_edge, true, stats);
    }

    /** The reference's defaults; dist_threshold = 0.05 x the trained model's diameter. */
    PPFClusterParams DefaultClusterParams() const {
        m3d_ppf_cluster_params p;
        m3d_ppf_default_cluster_params(model_, &p);
        return PPFClusterParams{p.dist_threshold, p.angle_threshold, p.ratio, p.score_thresh, p.rel_dist_sparse_thresh, p.num_result,
                                static_cast<RefineMethod>(p.refine_method), p.object_id};
    }

    /** ClusterPoses with PoseAverage (K1 - K6 of "PPF pose clustering"): poses row-major 4 x 4 each, as Vote returns them. */
    PoseClusters ClusterPoses(const double* poses, const uint32_t* num_votes, size_t n_poses, const PPFClusterParams& params,
                              int device = 0) const {
        const m3d_ppf_cluster_params p = params.c();
        PoseClusters out;
        size_t pcap = n_poses, ccap = 64, nv = 0, nt = 0, nr = 0;
        std::vector<double> avg;
        for (int attempt = 0; attempt < 2; ++attempt) {
            out.order.assign(pcap, 0);
            out.count_t.assign(pcap, 0);
            out.count_r.assign(pcap, 0);
            out.label_t.assign(pcap, -1);
            out.label_r.assign(pcap, -1);
            out.min_num_pt_r.assign(ccap, 0);
            out.cluster_votes.assign(ccap, 0);
            out.avg_votes.assign(ccap, 0);
            out.avg_cluster.assign(ccap, 0);
            avg.assign(16 * ccap, 0.0);
            const int rc = m3d_ppf_cluster_poses(poses, num_votes, n_poses, &p, device, pcap, &nv, out.order.data(), out.count_t.data(),
                                                 out.label_t.data(), out.count_r.data(), out.label_r.data(), ccap, &nt, &nr,
                                                 &out.min_num_pt_t, out.min_num_pt_r.data(), out.cluster_votes.data(), avg.data(),
                                                 out.avg_votes.data(), out.avg_cluster.data(), &out.stats);
            if (rc == M3D_ERR_CAPACITY && attempt == 0 && nv <= pcap) {
                ccap = nt > nr ? nt : nr;
                continue;
            }
            CheckStatus(rc);
            break;
        }
        for (auto* v : {&out.order, &out.count_t, &out.count_r}) v->resize(nv);
        out.label_t.resize(nv);
        out.label_r.resize(nv);
        out.min_num_pt_r.resize(nt);
        out.cluster_votes.resize(nt);
        out.avg_votes.resize(nr);
        out.avg_cluster.resize(nr);
        out.avg_poses.resize(nr);
        for (size_t k = 0; k < nr; ++k)
            for (int e = 0; e < 16; ++e) out.avg_poses[k][e] = avg[16 * k + e];
        return out;
    }

    /** Estimate from the vote on (:304-395): vote, cluster, average, refine, shift by the centroid, score; best first. */
    std::vector<Pose6D> Estimate(const double* scene_points, const double* scene_normals, size_t m, const std::vector<size_t>& reference,
                                 const PPFClusterParams& params, m3d_ppf_estimate_stats* stats = nullptr) const {
        return EstimateImpl(scene_points, scene_normals, m, reference, nullptr, nullptr, 0, false, params, stats);
    }

    /** Estimate of an EdgePoints model: the vote on the scene's edges, the refinement against the scene sample. */
    std::vector<Pose6D> EstimateEdges(const double* scene_points, const double* scene_normals, size_t m, const std::vector<size_t>& reference,
                                      const double* scene_edge_points, const double* scene_edge_normals, size_t m_edge,
                                      const PPFClusterParams& params, m3d_ppf_estimate_stats* stats = nullptr) const {
        return EstimateImpl(scene_points, scene_normals, m, reference, scene_edge_points, scene_edge_normals, m_edge, true, params, stats);
    }

    /** PreprocessEstimate (:243-278): normals may be null (then estimated); dist_step_dense <= 0: no edge part. */
    static PreparedScene PrepareScene(const double* points, const double* normals, size_t n, double diameter, double calc_normal_relative,
                                      double dist_step, double dist_step_dense = 0.0, int pts_num = 30, int device = 0) {
        PreparedScene out;
        const bool dense = dist_step_dense > 0.0;
        out.sample_points.resize(3 * n);
        out.sample_normals.resize(3 * n);
        out.dense_points.resize(dense ? 3 * n : 0);
        out.dense_normals.resize(dense ? 3 * n : 0);
        out.edge_indices.resize(dense ? n : 0);
        size_t ns = 0, nd = 0, ne = 0;
        CheckStatus(m3d_ppf_prepare_scene(points, normals, n, diameter, calc_normal_relative, dist_step, dist_step_dense, pts_num, device,
                                          out.sample_points.data(), out.sample_normals.data(), &ns, out.dense_points.data(),
                                          out.dense_normals.data(), &nd, out.edge_indices.data(), &ne));
        out.sample_points.resize(3 * ns);
        out.sample_normals.resize(3 * ns);
        out.dense_points.resize(3 * nd);
        out.dense_normals.resize(3 * nd);
        out.edge_indices.resize(ne);
        return out;
    }

private:
    std::vector<VotedPose> VoteImpl(const double* scene_points, const double* scene_normals, size_t m, const std::vector<size_t>& reference,
                                    const double* edge_points, const double* edge_normals, size_t m_edge, bool edges,
                                    m3d_ppf_vote_stats* stats) const {
        if (!model_) LogError("PPFVoting: not trained");
        size_t cap = reference.size() * 4 + 256, count = 0;
        std::vector<uint32_t> rp, mi, ai, nv;
        std::vector<double> poses;
        for (int attempt = 0; attempt < 2; ++attempt) {
            rp.assign(cap, 0);
            mi.assign(cap, 0);
            ai.assign(cap, 0);
            nv.assign(cap, 0);
            poses.assign(cap * 16, 0.0);
            const int rc = edges ? m3d_ppf_vote_edges(model_, scene_points, scene_normals, m, reference.data(), reference.size(), edge_points,
                                                      edge_normals, m_edge, cap, &count, rp.data(), mi.data(), ai.data(), nv.data(),
                                                      poses.data(), stats)
                                 : m3d_ppf_vote(model_, scene_points, scene_normals, m, reference.data(), reference.size(), cap, &count,
                                                rp.data(), mi.data(), ai.data(), nv.data(), poses.data(), stats);
            if (rc == M3D_ERR_CAPACITY && attempt == 0) {
                cap = count;
                continue;
            }
            CheckStatus(rc);
            break;
        }
        std::vector<VotedPose> out(count);
        for (size_t k = 0; k < count; ++k) {
            for (int t = 0; t < 16; ++t) out[k].pose[t] = poses[16 * k + t];
            out[k].num_votes = nv[k];
            out[k].corr_mi = mi[k];
            out[k].reference = rp[k];
            out[k].alpha_index = ai[k];
        }
        return out;
    }

    std::vector<Pose6D> EstimateImpl(const double* scene_points, const double* scene_normals, size_t m, const std::vector<size_t>& reference,
                                     const double* edge_points, const double* edge_normals, size_t m_edge, bool edges,
                                     const PPFClusterParams& params, m3d_ppf_estimate_stats* stats) const {
        if (!model_) LogError("PPFVoting: not trained");
        const m3d_ppf_cluster_params p = params.c();
        const size_t cap = params.num_result > 0 ? static_cast<size_t>(params.num_result) : 1;
        std::vector<double> poses(16 * cap), q(4 * cap), t(3 * cap), scores(cap);
        std::vector<uint64_t> votes(cap);
        size_t count = 0;
        CheckStatus(edges ? m3d_ppf_estimate_edges(model_, scene_points, scene_normals, m, reference.data(), reference.size(), edge_points,
                                                   edge_normals, m_edge, &p, cap, &count, poses.data(), q.data(), t.data(), votes.data(),
                                                   scores.data(), stats)
                          : m3d_ppf_estimate(model_, scene_points, scene_normals, m, reference.data(), reference.size(), &p, cap, &count,
                                             poses.data(), q.data(), t.data(), votes.data(), scores.data(), stats));
        std::vector<Pose6D> out(count);
        for (size_t k = 0; k < count; ++k) {
            for (int e = 0; e < 16; ++e) out[k].pose[e] = poses[16 * k + e];
            for (int e = 0; e < 4; ++e) out[k].q[e] = q[4 * k + e];
            for (int e = 0; e < 3; ++e) out[k].t[e] = t[3 * k + e];
            out[k].num_votes = static_cast<size_t>(votes[k]);
            out[k].score = scores[k];
            out[k].object_id = params.object_id;
        }
        return out;
    }

    void Reset() {
        if (model_) m3d_ppf_model_destroy(model_);
        model_ = nullptr;
    }
    m3d_ppf_model* model_ = nullptr;
};

}  // namespace pose_estimation
}  // namespace misc3d
