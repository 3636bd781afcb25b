// m3d_ppf_cluster.cpp -- ClusterPoses, PoseAverage, RefineSparsePose, the centre shift and the scoring of
// misc3d::pose_estimation::PPFEstimator (src/ppf_estimation.cpp) behind the C ABI: m3d_ppf_cluster_poses (K1 - K6) and
// m3d_ppf_estimate (the vote and K1 - K8).  The contract is in include/misc3d_amd.h "PPF pose clustering".  The device decides
// the neighbour counts, the cores and the labels of both levels (m3d_ppf_cluster.hip); the order, the cut, the ranking of the
// clusters, the averaging, the shift and the score are the host's, with the arithmetic of m3d_ppf_cluster_fp.hpp.  Nothing
// here depends on M3D_FP_ORDER (every sum is written out).
#include "m3d_driver_internal.hpp"
#include "m3d_ppf_cluster.hpp"

#include "../../include/misc3d_amd_bench.h"

#include <atomic>
#include <numeric>

#pragma clang fp contract(off)

using namespace m3d;

namespace {

std::atomic<int> g_pc_force_splits{0};   // m3d_bench_ppf_cluster_force

constexpr uint32_t kPcFillGroups = 256;   // row blocks below this: split the j tiles (one workgroup per CU)

// K1 - K6 of one call, as the host holds them
struct PcResult {
    std::vector<uint32_t> order, count_t, count_r;   // n_valid
    std::vector<int32_t> label_t, label_r;           // n_valid: ranks, -1 = dropped
    int32_t min_num_pt_t = 0;
    std::vector<int32_t> min_num_pt_r;               // per translation cluster
    std::vector<uint64_t> cluster_votes;             // per translation cluster
    std::vector<double> avg_poses;                   // 16 per sub-cluster, (translation cluster, sub-cluster) order
    std::vector<uint64_t> avg_votes;
    std::vector<uint32_t> avg_cluster;
    m3d_ppf_cluster_stats S{};
};

int pc_check_params(const m3d_ppf_cluster_params& P) {
    if (!(P.dist_threshold > 0.0) || !std::isfinite(P.dist_threshold))
        return fail(M3D_ERR_INVALID_ARG, "ppf cluster: dist_threshold must be positive and finite");
    if (!(P.angle_threshold > 0.0) || !(P.angle_threshold <= M_PI))
        return fail(M3D_ERR_INVALID_ARG, "ppf cluster: angle_threshold must be in (0, pi]");
    if (!std::isfinite(P.ratio) || !std::isfinite(P.score_thresh) || !std::isfinite(P.rel_dist_sparse_thresh) || !(P.ratio > 0.0))
        return fail(M3D_ERR_INVALID_ARG, "ppf cluster: ratio, score_thresh and rel_dist_sparse_thresh must be finite, ratio positive");
    if (P.refine_method != M3D_PPF_REFINE_NONE && P.refine_method != M3D_PPF_REFINE_POINT_TO_POINT &&
        P.refine_method != M3D_PPF_REFINE_POINT_TO_PLANE)
        return fail(M3D_ERR_INVALID_ARG, "ppf cluster: unknown refine_method");
    return M3D_OK;
}

// Ranks the clusters of one level.  root[i]: the device's label (the lowest core index of the cluster, or kPcNone); outer[i]:
// the rank of the enclosing translation cluster (level 2) or 0 (level 1).  Clusters are ordered by (outer, votes descending,
// lowest member); rank[i] = the position of i's cluster among those of its outer cluster.  -> the clusters in that order.
struct PcCluster {
    uint32_t root, lowest, outer;
    uint64_t votes;
};
std::vector<PcCluster> pc_rank(const std::vector<uint32_t>& root, const std::vector<int32_t>& outer, const uint32_t* votes,
                               std::vector<int32_t>* rank) {
    const size_t n = root.size();
    std::vector<int32_t> slot(n, -1);
    std::vector<PcCluster> found;
    for (size_t i = 0; i < n; ++i) {
        if (root[i] == kPcNone) continue;
        int32_t& s = slot[root[i]];
        if (s < 0) {
            s = (int32_t)found.size();
            found.push_back({root[i], (uint32_t)i, (uint32_t)outer[i], 0});
        }
        found[(size_t)s].votes += votes[i];
    }
    std::vector<uint32_t> by(found.size());
    std::iota(by.begin(), by.end(), 0u);
    std::sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) {
        const PcCluster &x = found[a], &y = found[b];
        if (x.outer != y.outer) return x.outer < y.outer;
        if (x.votes != y.votes) return x.votes > y.votes;
        return x.lowest < y.lowest;
    });
    std::vector<PcCluster> sorted(found.size());
    std::vector<int32_t> rank_of_slot(found.size());
    uint32_t in_outer = 0;
    for (size_t k = 0; k < by.size(); ++k) {
        sorted[k] = found[by[k]];
        in_outer = (k && sorted[k].outer == sorted[k - 1].outer) ? in_outer + 1 : 0;
        rank_of_slot[by[k]] = (int32_t)in_outer;
    }
    rank->assign(n, -1);
    for (size_t i = 0; i < n; ++i)
        if (root[i] != kPcNone) (*rank)[i] = rank_of_slot[(size_t)slot[root[i]]];
    return sorted;
}

// K1 - K6 on a lane the caller holds.  poses / votes: the caller's P raw poses, every entry finite.
int pc_cluster_on(DeviceCtx* ctx, const double* poses, const uint32_t* votes, size_t P, const m3d_ppf_cluster_params& prm, PcResult* R) {
    const double t0 = now_ms();
    if (P == 0) {
        R->S.ms_total = now_ms() - t0;
        return M3D_OK;
    }
    // K1, K2
    std::vector<uint32_t> order(P);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return votes[a] > votes[b]; });
    const size_t threshold = (size_t)((double)votes[order[0]] * 0.5);
    size_t V = 0;
    while (V < P && votes[order[V]] >= threshold) ++V;
    R->S.n_valid = V;
    if (V > kPcMaxValid)
        return fail(M3D_ERR_CAPACITY, "ppf cluster: " + std::to_string(V) + " valid poses, one call clusters at most " + std::to_string(kPcMaxValid));
    order.resize(V);
    const uint32_t n = (uint32_t)V;
    std::vector<double> soa((size_t)kPcRows * n);
    std::vector<uint32_t> sv(n);
    for (uint32_t i = 0; i < n; ++i) {
        const double* T = poses + 16 * (size_t)order[i];
        for (int a = 0; a < 3; ++a) soa[(size_t)a * n + i] = T[4 * a + 3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) soa[(size_t)(3 + 3 * r + c) * n + i] = T[4 * r + c];
        sv[i] = votes[order[i]];
    }
    const uint32_t rows = (n + kPcTile - 1) / kPcTile;
    uint32_t splits = rows < kPcFillGroups ? (kPcFillGroups + rows - 1) / rows : 1;
    if (const int f = g_pc_force_splits.load(); f > 0) splits = (uint32_t)f;
    splits = std::min(splits, rows);
    R->S.splits = splits;
    // the device's integers, one block: count_t, label_t, count_r, label_r, max_r (n words each), max_t (1 word)
    const size_t words = 5 * (size_t)n + 1;
    std::vector<uint32_t> back(words);
    DevBuf d_pose, d_ints, d_core, d_parent;
    const int rc = [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        RESERVE(d_pose, sizeof(double) * soa.size());
        RESERVE(d_ints, sizeof(uint32_t) * words);
        RESERVE(d_core, sizeof(uint32_t) * n);
        RESERVE(d_parent, sizeof(uint32_t) * n);
        HIPCHK(hipEventRecord(ctx->ev0, st));
        HIPCHK(hipMemcpyAsync(d_pose.p, soa.data(), sizeof(double) * soa.size(), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(d_ints.p, 0, sizeof(uint32_t) * words, st));
        uint32_t* w = d_ints.as<uint32_t>();
        PcLevel L;
        L.pose = d_pose.as<double>();
        L.n = n;
        L.r2 = prm.dist_threshold * prm.dist_threshold;
        L.cos_edge = std::cos(prm.angle_threshold);
        L.group = nullptr;
        L.count = w;
        L.max_count = w + 5 * (size_t)n;
        L.core = d_core.as<uint32_t>();
        L.parent = d_parent.as<uint32_t>();
        L.label = w + n;
        launch_pc_level(L, 1, splits, st);
        L.group = w + n;
        L.count = w + 2 * (size_t)n;
        L.max_count = w + 4 * (size_t)n;
        L.label = w + 3 * (size_t)n;
        launch_pc_level(L, 2, splits, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(back.data(), d_ints.p, sizeof(uint32_t) * words, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(ctx->ev1, st));
        HIPCHK(hipEventSynchronize(ctx->ev1));
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        R->S.ms_device = ms;
        return M3D_OK;
    }();
    (void)hipStreamSynchronize(ctx->stream);
    for (DevBuf* b : {&d_pose, &d_ints, &d_core, &d_parent}) b->release();
    if (rc != M3D_OK) return rc;
    R->S.launches = 2 * kPcLaunchesPerLevel;
    R->S.pair_tests = (uint64_t)(2 * kPcPairKernelsPerLevel) * n * n;

    const uint32_t *c_t = back.data(), *l_t = c_t + n, *c_r = l_t + n, *l_r = c_r + n, *max_r = l_r + n;
    const uint32_t max_t = back[5 * (size_t)n];
    for (uint32_t i = 0; i < n; ++i) {   // self-check: a label is a pose of the call, and a level-2 label lies in a level-1 cluster
        const bool bad_t = l_t[i] != kPcNone && l_t[i] >= n;
        const bool bad_r = l_r[i] != kPcNone && (l_r[i] >= n || l_t[i] == kPcNone);
        if (bad_t || bad_r || c_t[i] == 0 || c_t[i] > n) return fail(M3D_ERR_INTERNAL, "ppf cluster: a label or count is out of range (self-check)");
    }
    R->order = order;
    R->count_t.assign(c_t, c_t + n);
    R->count_r.assign(c_r, c_r + n);
    R->min_num_pt_t = (int32_t)pc_min_num_pt(max_t);
    // K4: the translation clusters, ranked
    const std::vector<uint32_t> root_t(l_t, l_t + n), root_r(l_r, l_r + n);
    const std::vector<PcCluster> ct = pc_rank(root_t, std::vector<int32_t>(n, 0), sv.data(), &R->label_t);
    R->min_num_pt_r.resize(ct.size());
    R->cluster_votes.resize(ct.size());
    for (size_t c = 0; c < ct.size(); ++c) {
        R->min_num_pt_r[c] = (int32_t)pc_min_num_pt(max_r[ct[c].root]);
        R->cluster_votes[c] = ct[c].votes;
    }
    // K5: the sub-clusters, ranked inside their translation clusters; K6: their averages, members ascending
    std::vector<int32_t> outer(n, 0);
    for (uint32_t i = 0; i < n; ++i) outer[i] = R->label_t[i] < 0 ? 0 : R->label_t[i];
    const std::vector<PcCluster> cr = pc_rank(root_r, outer, sv.data(), &R->label_r);
    std::vector<size_t> first_of(ct.size() + 1, 0);   // the first averaged pose of every translation cluster
    for (const PcCluster& c : cr) first_of[c.outer + 1] += 1;
    for (size_t c = 0; c < ct.size(); ++c) first_of[c + 1] += first_of[c];
    std::vector<pc_avg_sums> sums(cr.size());
    for (pc_avg_sums& s : sums) pc_avg_clear(&s);
    for (uint32_t i = 0; i < n; ++i)
        if (R->label_r[i] >= 0)
            pc_avg_add(&sums[first_of[(size_t)R->label_t[i]] + (size_t)R->label_r[i]], poses + 16 * (size_t)order[i], sv[i]);
    R->avg_poses.resize(16 * cr.size());
    R->avg_votes.resize(cr.size());
    R->avg_cluster.resize(cr.size());
    for (size_t k = 0; k < cr.size(); ++k) {
        pc_avg_pose(&sums[k], &R->avg_poses[16 * k], nullptr);
        R->avg_votes[k] = sums[k].votes;
        R->avg_cluster[k] = cr[k].outer;
        if (sums[k].votes != cr[k].votes) return fail(M3D_ERR_INTERNAL, "ppf cluster: a sub-cluster's votes disagree (self-check)");
    }
    R->S.clusters_t = ct.size();
    R->S.clusters_r = cr.size();
    R->S.ms_total = now_ms() - t0;
    return M3D_OK;
}

}  // namespace

namespace {

// m3d_ppf_estimate's result arrays, `capacity` entries each
struct PpfEstimateOut {
    size_t capacity;
    size_t* n_results;
    double *poses, *q, *t;
    uint64_t* votes;
    double* scores;
};

// Estimate from the vote on (:304-395), the vote, the clustering and the refinement on one lane.  With scene.edges (rule E9) the
// vote reads the scene's edge points, the refinement still runs against the scene sample, and K8's expected votes drop the 0.25.
int ppf_estimate(const m3d_ppf_model* model, const PpfScene& scene, const m3d_ppf_cluster_params* params, const PpfEstimateOut& out,
                 m3d_ppf_estimate_stats* stats) {
    const double t0 = now_ms();
    m3d_ppf_estimate_stats S{};
    if (stats) *stats = S;
    if (out.n_results) *out.n_results = 0;
    if (!model || !out.n_results) return fail(M3D_ERR_INVALID_ARG, "ppf estimate: null argument");
    if (out.capacity && (!out.poses || !out.q || !out.t || !out.votes || !out.scores))
        return fail(M3D_ERR_INVALID_ARG, "ppf estimate: null result array");
    m3d_ppf_cluster_params prm;
    m3d_ppf_default_cluster_params(model, &prm);
    if (params) prm = *params;
    if (const int rc = pc_check_params(prm); rc != M3D_OK) return rc;
    const PpfModelHost M = ppf_model_host(model);
    const double *scene_points = scene.sample.pts, *scene_normals = scene.sample.nrm;
    const size_t m = scene.sample.n;
    // the vote's own checks of the scene and the reference indices, in front of the lane
    const double tv = now_ms();
    PpfVote V;
    if (const int rc = ppf_check_vote(model, scene, nullptr, &V); rc != M3D_OK) return rc;
    struct Result {
        double T[16];
        uint64_t votes;
    };
    std::vector<Result> results;
    LaneLock lane(M.device);   // one lane, one configuration snapshot: the vote, the clustering and every ICP call run on it
    if (!lane.ctx) return M3D_ERR_DEVICE;
    if (const int rc = ppf_vote_on(lane.ctx, model, scene, &V); rc != M3D_OK) return rc;
    V.stats.ms_total = now_ms() - tv;
    S.vote = V.stats;
    S.ms_vote = V.stats.ms_total;
    const size_t n_raw = V.maxima.size();
    S.n_raw = n_raw;
    if (n_raw) {
        std::vector<uint32_t> raw_votes(n_raw);
        std::vector<double> raw_poses(16 * n_raw);
        for (size_t k = 0; k < n_raw; ++k) {
            raw_votes[k] = V.maxima[k].votes;
            ppf_vote_pose(model, V, k, &raw_poses[16 * k]);
        }
        PcResult R;
        const double tc = now_ms();
        if (const int rc = pc_cluster_on(lane.ctx, raw_poses.data(), raw_votes.data(), n_raw, prm, &R); rc != M3D_OK) return rc;
        S.cluster = R.S;
        S.ms_cluster = now_ms() - tc;
        // K7: per translation cluster with a sub-cluster, the averaged pose with the most votes (the first on ties)
        const double tr = now_ms();
        const double max_dist = prm.rel_dist_sparse_thresh * M.dist_step;
        for (size_t k = 0; k < R.avg_votes.size();) {
            size_t end = k, best = k;
            while (end < R.avg_votes.size() && R.avg_cluster[end] == R.avg_cluster[k]) {
                if (R.avg_votes[end] > R.avg_votes[best]) best = end;
                ++end;
            }
            Result res;
            std::memcpy(res.T, &R.avg_poses[16 * best], sizeof(res.T));
            res.votes = R.avg_votes[best];
            if (prm.refine_method != M3D_PPF_REFINE_NONE) {
                double T_out[16];
                m3d_icp_stats is{};
                const int rc = prm.refine_method == M3D_PPF_REFINE_POINT_TO_POINT
                                   ? registration_icp_on(lane.ctx, M.centred, M.n, scene_points, m, max_dist, res.T, 30, 1e-6, 1e-6, M.device,
                                                         T_out, &is, nullptr)
                                   : registration_icp_plane_on(lane.ctx, M.centred, M.n, scene_points, scene_normals, m, max_dist, res.T, 30,
                                                               1e-6, 1e-6, M.device, T_out, &is, nullptr, true);
                if (rc != M3D_OK) return rc;
                std::memcpy(res.T, T_out, sizeof(res.T));
                S.icp_calls += 1;
                S.icp_iterations += (uint32_t)is.iterations;
            }
            results.push_back(res);
            k = end;
        }
        S.ms_refine = now_ms() - tr;
    }
    // K8
    for (Result& r : results) pc_centre_shift(r.T, M.centroid);
    std::stable_sort(results.begin(), results.end(), [](const Result& a, const Result& b) { return a.votes > b.votes; });
    const double expected = scene.edges ? pc_expected_votes_edges(prm.ratio, M.n) : pc_expected_votes(prm.ratio, M.n);
    size_t keep = 0;
    while (keep < results.size() && !(pc_score(results[keep].votes, expected) < prm.score_thresh)) ++keep;
    if (prm.num_result >= 0 && keep > (size_t)prm.num_result) keep = (size_t)prm.num_result;
    *out.n_results = keep;
    S.ms_total = now_ms() - t0;
    S.ms_host = S.ms_total - S.ms_vote - S.ms_cluster - S.ms_refine;
    if (stats) *stats = S;
    if (keep > out.capacity)
        return fail(M3D_ERR_CAPACITY, "ppf estimate: " + std::to_string(keep) + " results, the result arrays hold " + std::to_string(out.capacity));
    for (size_t k = 0; k < keep; ++k) {
        double Rm[9];
        std::memcpy(out.poses + 16 * k, results[k].T, sizeof(double) * 16);
        pc_pose_rotation(results[k].T, Rm);
        pc_mat_to_quat(Rm, out.q + 4 * k);
        for (int a = 0; a < 3; ++a) out.t[3 * k + a] = results[k].T[4 * a + 3];
        out.votes[k] = results[k].votes;
        out.scores[k] = pc_score(results[k].votes, expected);
    }
    return M3D_OK;
}

}  // namespace

extern "C" {

void m3d_ppf_default_cluster_params(const m3d_ppf_model* model, m3d_ppf_cluster_params* out) {
    if (!out) return;
    out->dist_threshold = 0.05 * (model ? ppf_model_host(model).diameter : 1.0);
    out->angle_threshold = 12.0 / 180.0 * M_PI;
    out->ratio = 0.6;
    out->score_thresh = 0.6;
    out->rel_dist_sparse_thresh = 5.0;
    out->num_result = 10;
    out->refine_method = M3D_PPF_REFINE_POINT_TO_PLANE;
    out->object_id = 0;
    out->reserved = 0;
}

int m3d_ppf_cluster_poses(const double* poses, const uint32_t* votes, size_t P, const m3d_ppf_cluster_params* params, int device,
                          size_t pose_capacity, size_t* n_valid, uint32_t* order, uint32_t* count_t, int32_t* label_t,
                          uint32_t* count_r, int32_t* label_r, size_t cluster_capacity, size_t* n_clusters_t, size_t* n_clusters_r,
                          int32_t* min_num_pt_t, int32_t* min_num_pt_r, uint64_t* cluster_votes, double* avg_poses,
                          uint64_t* avg_votes, uint32_t* avg_cluster, m3d_ppf_cluster_stats* stats) {
    m3d_ppf_cluster_stats S{};
    if (stats) *stats = S;
    if (n_valid) *n_valid = 0;
    if (n_clusters_t) *n_clusters_t = 0;
    if (n_clusters_r) *n_clusters_r = 0;
    if (!params || !n_valid || !n_clusters_t || !n_clusters_r) return fail(M3D_ERR_INVALID_ARG, "ppf cluster: null argument");
    if (P && (!poses || !votes)) return fail(M3D_ERR_INVALID_ARG, "ppf cluster: null poses or votes");
    if (P >= ((size_t)1 << 31)) return fail(M3D_ERR_INVALID_ARG, "ppf cluster: at most 2^31 - 1 poses");
    if (pose_capacity && (!order || !count_t || !label_t || !count_r || !label_r)) return fail(M3D_ERR_INVALID_ARG, "ppf cluster: null per-pose array");
    if (cluster_capacity && (!min_num_pt_r || !cluster_votes || !avg_poses || !avg_votes || !avg_cluster))
        return fail(M3D_ERR_INVALID_ARG, "ppf cluster: null per-cluster array");
    if (const int rc = pc_check_params(*params); rc != M3D_OK) return rc;
    for (size_t k = 0; k < 16 * P; ++k)
        if (!std::isfinite(poses[k])) return fail(M3D_ERR_INVALID_ARG, "ppf cluster: a pose entry is not finite");
    if (P == 0) return M3D_OK;
    PcResult R;
    int rc;
    {
        LaneLock lane(device);
        if (!lane.ctx) return M3D_ERR_DEVICE;
        rc = pc_cluster_on(lane.ctx, poses, votes, P, *params, &R);
    }
    *n_valid = (size_t)R.S.n_valid;
    if (rc != M3D_OK) return rc;
    *n_clusters_t = (size_t)R.S.clusters_t;
    *n_clusters_r = (size_t)R.S.clusters_r;
    if (stats) *stats = R.S;
    if (min_num_pt_t) *min_num_pt_t = R.min_num_pt_t;
    if (R.S.n_valid > pose_capacity || std::max(R.S.clusters_t, R.S.clusters_r) > cluster_capacity)
        return fail(M3D_ERR_CAPACITY, "ppf cluster: " + std::to_string(R.S.n_valid) + " valid poses, " + std::to_string(R.S.clusters_t) +
                                          " + " + std::to_string(R.S.clusters_r) + " clusters: the result arrays hold " +
                                          std::to_string(pose_capacity) + " and " + std::to_string(cluster_capacity));
    const size_t n = R.order.size(), ct = R.cluster_votes.size(), cr = R.avg_votes.size();
    if (n) {
        std::memcpy(order, R.order.data(), sizeof(uint32_t) * n);
        std::memcpy(count_t, R.count_t.data(), sizeof(uint32_t) * n);
        std::memcpy(label_t, R.label_t.data(), sizeof(int32_t) * n);
        std::memcpy(count_r, R.count_r.data(), sizeof(uint32_t) * n);
        std::memcpy(label_r, R.label_r.data(), sizeof(int32_t) * n);
    }
    if (ct) {
        std::memcpy(min_num_pt_r, R.min_num_pt_r.data(), sizeof(int32_t) * ct);
        std::memcpy(cluster_votes, R.cluster_votes.data(), sizeof(uint64_t) * ct);
    }
    if (cr) {
        std::memcpy(avg_poses, R.avg_poses.data(), sizeof(double) * 16 * cr);
        std::memcpy(avg_votes, R.avg_votes.data(), sizeof(uint64_t) * cr);
        std::memcpy(avg_cluster, R.avg_cluster.data(), sizeof(uint32_t) * cr);
    }
    return M3D_OK;
}

int m3d_ppf_estimate(const m3d_ppf_model* model, const double* scene_points, const double* scene_normals, size_t m,
                     const size_t* reference, size_t n_ref, const m3d_ppf_cluster_params* params, size_t capacity,
                     size_t* n_results, double* poses, double* q, double* t, uint64_t* votes, double* scores,
                     m3d_ppf_estimate_stats* stats) {
    return ppf_estimate(model, {{scene_points, scene_normals, m}, reference, n_ref, nullptr}, params,
                        {capacity, n_results, poses, q, t, votes, scores}, stats);
}

int m3d_ppf_estimate_edges(const m3d_ppf_model* model, const double* scene_points, const double* scene_normals, size_t m,
                           const size_t* reference, size_t n_ref, const double* scene_edge_points, const double* scene_edge_normals,
                           size_t m_edge, const m3d_ppf_cluster_params* params, size_t capacity, size_t* n_results, double* poses,
                           double* q, double* t, uint64_t* votes, double* scores, m3d_ppf_estimate_stats* stats) {
    const PpfCloud edges{scene_edge_points, scene_edge_normals, m_edge};
    return ppf_estimate(model, {{scene_points, scene_normals, m}, reference, n_ref, &edges}, params,
                        {capacity, n_results, poses, q, t, votes, scores}, stats);
}

// measurement / test hook (include/misc3d_amd_bench.h)
int m3d_bench_ppf_cluster_force(int splits) {
    if (splits < 0) return fail(M3D_ERR_INVALID_ARG, "ppf cluster: splits must be >= 0");
    g_pc_force_splits.store(splits);
    return M3D_OK;
}

}  // extern "C"
