// m3d_ppf_train.cpp -- m3d_ppf_prepare_model: PPFEstimator::PreprocessTrain (src/ppf_estimation.cpp:206-241 with :1063-1160) as a
// host composition of calls this library has (m3d_estimate_normals, m3d_orient_normals_mst, m3d_detect_boundary_points) on ONE lane
// of the device, held from the first of them to the last, with the host steps of m3d_ppf_train.hpp between them, and m3d_ppf_reference_indices (Estimate's reference points).
// The contract is the block "PPF model preprocessing" of include/misc3d_amd.h.
#include "m3d_ppf_train.hpp"

#include "../../include/misc3d_amd.h"
#include "m3d_host_util.hpp"

#include <string>

#pragma clang fp contract(off)

extern "C" void m3d_ppf_train_params_default_(m3d_ppf_train_params* p) {
    if (!p) return;
    *p = m3d_ppf_train_params{};
    p->rel_sample_dist = 0.05;
    p->rel_dense_sample_dist = 0.025;
    p->calc_normal_relative = 0.01;
    p->pts_num = 20;
}

extern "C" int m3d_ppf_prepare_model(const double* xyz, const double* normals, size_t n, const m3d_ppf_train_params* params,
                                     const double* box_center, const double* box_extent, int device, double* out_normals,
                                     size_t* sample_indices, size_t* n_sample, size_t* dense_indices, size_t* n_dense,
                                     size_t* edge_indices, size_t* n_edges, m3d_ppf_model_info* info) {
    using namespace m3d;
    const double t0 = now_ms();
    if (n_sample) *n_sample = 0;
    if (n_dense) *n_dense = 0;
    if (n_edges) *n_edges = 0;
    if (info) *info = m3d_ppf_model_info{};
    if (!params || !n_sample || !n_dense || !n_edges) return fail(M3D_ERR_INVALID_ARG, "ppf prepare model: null argument");
    if (n == 0) return fail(M3D_ERR_INVALID_ARG, "There is no input points");
    if (n >= ((size_t)1 << 31)) return fail(M3D_ERR_INVALID_ARG, "too many points");
    const bool dense = params->rel_dense_sample_dist > 0.0;
    if (!xyz || !out_normals || !sample_indices || (dense && (!dense_indices || !edge_indices)) || !box_center != !box_extent)
        return fail(M3D_ERR_INVALID_ARG, "ppf prepare model: null array");
    for (size_t k = 0; k < 3 * n; ++k)
        if (!std::isfinite(xyz[k])) return fail(M3D_ERR_INVALID_ARG, "ppf prepare model: point " + std::to_string(k / 3) + " is not finite");
    m3d_ppf_model_info I{};
    // B1, B2
    TrainBox box;
    if (box_center) {
        for (int k = 0; k < 3; ++k) {
            box.center[k] = box_center[k];
            box.extent[k] = box_extent[k];
        }
    } else {
        box = train_box(xyz, n);
    }
    const TrainDerived d = train_derive(box, params->rel_sample_dist, params->rel_dense_sample_dist, params->calc_normal_relative);
    for (int k = 0; k < 3; ++k) {
        I.box_center[k] = box.center[k];
        I.box_extent[k] = box.extent[k];
        I.view_pt[k] = d.view_pt[k];
    }
    I.diameter = d.diameter;
    I.r_min = d.r_min;
    I.dist_step = d.dist_step;
    I.dist_step_dense = d.dist_step_dense;
    I.normal_r = d.normal_r;
    I.ms_box = now_ms() - t0;
    if (!std::isfinite(d.normal_r) || !(d.normal_r > 0.0) || !(d.dist_step > 0.0))
        return fail(M3D_ERR_INVALID_ARG, "ppf prepare model: the box gives no positive search radius and sample distance");
    LaneLock lane(device);   // normals, orientation and boundary detection run on this lane
    DeviceCtx* ctx = lane.ctx;
    if (!ctx) return M3D_ERR_DEVICE;
    // B3
    double t1 = now_ms();
    std::vector<double> nrm(3 * n);
    if (normals) {
        std::copy(normals, normals + 3 * n, nrm.begin());
    } else if (const int rc = estimate_normals_on(ctx, xyz, n, 2, d.normal_r, 30, 0, nullptr, device, nrm.data(), nullptr); rc != M3D_OK) {
        return rc;
    }
    train_normalize(nrm.data(), n);
    // B4
    const size_t seed = train_seed(xyz, n, d.view_pt);
    I.seed = seed;
    if (!(normals && params->use_external_normal)) {
        if (train_seed_flips(xyz + 3 * seed, nrm.data() + 3 * seed, d.view_pt, params->invert_model_normal != 0)) {
            for (int k = 0; k < 3; ++k) nrm[3 * seed + k] = -nrm[3 * seed + k];
            I.seed_flipped = 1;
        }
        std::vector<int64_t> parent(n);
        if (const int rc = orient_normals_mst_on(ctx, xyz, nrm.data(), n, d.normal_r, seed, out_normals, parent.data(), &I.orient);
            rc != M3D_OK)
            return rc;
        I.oriented = 1;
    } else {
        std::copy(nrm.begin(), nrm.end(), out_normals);
    }
    I.ms_normals = now_ms() - t1;
    // B5, B6
    t1 = now_ms();
    std::vector<size_t> sel;
    TrainSampleStats ss;
    train_sample(xyz, n, d.dist_step, seed, &sel, &ss);
    std::copy(sel.begin(), sel.end(), sample_indices);
    *n_sample = sel.size();
    I.sample_distance_evaluations = ss.distance_evaluations;
    I.ms_sample = now_ms() - t1;
    if (dense) {
        t1 = now_ms();
        train_sample(xyz, n, d.dist_step_dense, seed, &sel, &ss);
        std::copy(sel.begin(), sel.end(), dense_indices);
        *n_dense = sel.size();
        I.dense_distance_evaluations = ss.distance_evaluations;
        I.ms_dense = now_ms() - t1;
        t1 = now_ms();
        std::vector<double> dp(3 * sel.size()), dn(3 * sel.size());
        for (size_t k = 0; k < sel.size(); ++k)
            for (int a = 0; a < 3; ++a) {
                dp[3 * k + a] = xyz[3 * sel[k] + a];
                dn[3 * k + a] = out_normals[3 * sel[k] + a];
            }
        if (const int rc = detect_boundary_points_on(ctx, dp.data(), dn.data(), sel.size(), 2, d.normal_r, params->pts_num, 90.0, device,
                                                     edge_indices, n_edges);
            rc != M3D_OK) {
            *n_edges = 0;
            return rc;
        }
        I.ms_edges = now_ms() - t1;
    }
    I.ms_total = now_ms() - t0;
    if (info) *info = I;
    return M3D_OK;
}

extern "C" int m3d_ppf_reference_indices(size_t num, size_t sample, uint32_t seed, size_t* out) {
    using namespace m3d;
    if (num == 0 || num >= ((size_t)1 << 32) || sample > num) return fail(M3D_ERR_INVALID_ARG, "ppf reference indices: sample <= num < 2^32, num > 0");
    if (sample && !out) return fail(M3D_ERR_INVALID_ARG, "ppf reference indices: null array");
    train_reference_indices(num, sample, seed, out);
    return M3D_OK;
}
