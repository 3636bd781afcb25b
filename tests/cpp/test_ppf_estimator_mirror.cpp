// test_ppf_estimator_mirror.cpp -- include/misc3d/pose_estimation/ppf_estimation.h compiled with g++ against the library: the
// config's defaults, CheckConfig, the paths of Train / Estimate that end before any device is touched, and the host-only
// m3d_ppf_reference_indices.  No GPU.  Prints "ok" and returns 0, or the first failures and 1.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>

#include <misc3d/pose_estimation/ppf_estimation.h>

using namespace misc3d::pose_estimation;

static int g_fail = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond) && ++g_fail < 20) std::printf("line %d: %s\n", __LINE__, #cond); \
    } while (0)

template <class F>
static bool throws(F f, const char* text) {
    try {
        f();
    } catch (const std::runtime_error& e) {
        return std::string(e.what()).find(text) != std::string::npos;
    }
    return false;
}

int main() {
    misc3d::SetVerbosityLevel(misc3d::VerbosityLevel::Error);
    PPFEstimatorConfig c;
    CHECK(!c.training_param_.invert_model_normal && !c.training_param_.use_external_normal);
    CHECK(c.training_param_.rel_sample_dist == 0.05 && c.training_param_.rel_dense_sample_dist == 0.025);
    CHECK(c.training_param_.calc_normal_relative == 0.01 && c.ref_param_.ratio == 0.6);
    CHECK(c.voting_param_.method == PPFEstimatorConfig::VotingMode::SampledPoints && c.voting_param_.faster_mode);
    CHECK(c.voting_param_.angle_step == 12.0 / 180 * M_PI && c.voting_param_.min_angle_thresh == 30.0 / 180 * M_PI);
    CHECK(c.voting_param_.min_dist_thresh == 1.0 / 3 && c.edge_param_.pts_num == 20);
    CHECK(c.refine_param_.method == PPFEstimatorConfig::RefineMethod::PointToPlane && c.refine_param_.rel_dist_sparse_thresh == 5);
    CHECK(c.rel_dist_thresh_ == 0.05 && c.rel_angle_thresh_ == 12.0 / 180 * M_PI && c.score_thresh_ == 0.6);
    CHECK(c.num_result_ == 10 && c.object_id_ == 0);
    m3d_ppf_train_params tp;
    m3d_ppf_train_params_default_(&tp);
    CHECK(tp.rel_sample_dist == 0.05 && tp.rel_dense_sample_dist == 0.025 && tp.calc_normal_relative == 0.01 && tp.pts_num == 20);
    CHECK(!tp.invert_model_normal && !tp.use_external_normal);

    PPFEstimator e(c);
    CHECK(PPFEstimator::CheckConfig(c));
    PPFEstimatorConfig bad = c;
    bad.training_param_.rel_dense_sample_dist = 0.05;   // dense >= sparse
    // the reference's LogError throws (misc3d/logging.h): its messages arrive as std::runtime_error
    CHECK(throws([&] { PPFEstimator::CheckConfig(bad); }, "Dense_sample_dist should be smaller than sample_dist."));
    CHECK(throws([&] { e.SetConfig(bad); }, "Dense_sample_dist"));
    std::vector<Pose6D> results(3);
    const double one[3] = {0, 0, 0};
    CHECK(throws([&] { e.Estimate(misc3d::CloudView(one, nullptr, 1), results); }, "Need training before estimating!") && results.empty());
    CHECK(throws([&] { e.Train(misc3d::CloudView(nullptr, nullptr, 0)); }, "There is no input points"));
    CHECK(e.GetModelDiameter() == 0.0 && e.GetPose().empty() && e.GetSampledModel().points_.empty());

    size_t idx[6];
    CHECK(m3d_ppf_reference_indices(10, 6, 7, idx) == M3D_OK);
    bool distinct = true;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < i; ++j) distinct = distinct && idx[i] != idx[j] && idx[i] < 10;
    CHECK(distinct);
    CHECK(m3d_ppf_reference_indices(5, 6, 7, idx) == M3D_ERR_INVALID_ARG);
    if (g_fail) {
        std::printf("%d failures\n", g_fail);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
