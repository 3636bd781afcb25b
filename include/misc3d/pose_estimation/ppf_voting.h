// misc3d/pose_estimation/ppf_voting.h -- host mirror over the C ABI (m3d_ppf_*) of the two device hot paths of the
// reference's PPFEstimator (src/ppf_estimation.cpp): the point-pair table of a model (CalcHashTable, :603-640) and the vote of
// a scene against it (VotingAndGetPose, :399-524).  Header-only; no Eigen / Open3D needed.
//
// Both take ALREADY SAMPLED points with unit normals.  PreprocessTrain / PreprocessEstimate, ClusterPoses / PoseAverage, the
// EdgePoints mode, the scoring and the PPFEstimator class itself are not part of this build; the contract of what is here is
// written down next to m3d_ppf_vote in include/misc3d_amd.h.
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
    bool IsTrained() const { return model_ != nullptr; }
    size_t Size() const { return m3d_ppf_model_size(model_); }
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
            const int rc = m3d_ppf_vote(model_, scene_points, scene_normals, m, reference.data(), reference.size(), cap, &count,
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

private:
    void Reset() {
        if (model_) m3d_ppf_model_destroy(model_);
        model_ = nullptr;
    }
    m3d_ppf_model* model_ = nullptr;
};

}  // namespace pose_estimation
}  // namespace misc3d
