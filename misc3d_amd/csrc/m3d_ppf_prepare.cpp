// m3d_ppf_prepare.cpp -- m3d_ppf_prepare_scene: PPFEstimator::PreprocessEstimate (src/ppf_estimation.cpp:243-278) as a host
// composition of calls this library already has (m3d_estimate_normals, m3d_voxel_down_sample, m3d_detect_boundary_points) on
// one device; no kernel of its own.  The contract is in include/misc3d_amd.h; the two host steps are m3d_ppf_prepare.hpp's.
#include "m3d_ppf_prepare.hpp"

#include "../../include/misc3d_amd.h"

#include <string>

#pragma clang fp contract(off)

namespace m3d {
int fail(int code, const std::string& msg);
}

extern "C" int m3d_ppf_prepare_scene(const double* xyz, const double* normals, size_t n, double diameter, double calc_normal_relative,
                                     double dist_step, double dist_step_dense, int pts_num, int device, double* sample_xyz,
                                     double* sample_normals, size_t* n_sample, double* dense_xyz, double* dense_normals,
                                     size_t* n_dense, size_t* edge_indices, size_t* n_edges) {
    using m3d::fail;
    if (n_sample) *n_sample = 0;
    if (n_dense) *n_dense = 0;
    if (n_edges) *n_edges = 0;
    const bool dense = dist_step_dense > 0.0;
    if (!n_sample || !n_dense || !n_edges) return fail(M3D_ERR_INVALID_ARG, "ppf prepare: null count");
    if (n == 0) return fail(M3D_ERR_INVALID_ARG, "There is no scene point clouds.");
    if (!xyz || !sample_xyz || !sample_normals || (dense && (!dense_xyz || !dense_normals || !edge_indices)))
        return fail(M3D_ERR_INVALID_ARG, "ppf prepare: null array");
    std::vector<double> pts, nrm;
    const size_t k = m3d::ppf_drop_non_finite(xyz, normals, n, &pts, &nrm);   // step 1
    if (k == 0) return fail(M3D_ERR_INVALID_ARG, "There is no scene point clouds.");
    const double radius = calc_normal_relative * diameter;
    if (!normals) {   // step 2
        nrm.resize(3 * k);
        if (const int rc = m3d_estimate_normals(pts.data(), k, 2, radius, 30, 0, nullptr, device, nrm.data(), nullptr); rc != M3D_OK) return rc;
    }
    m3d::ppf_normal_consistent(pts.data(), nrm.data(), k);   // step 3
    if (const int rc = m3d_voxel_down_sample(pts.data(), nrm.data(), nullptr, k, dist_step, device, sample_xyz, sample_normals, nullptr,
                                             nullptr, nullptr, n_sample, nullptr);
        rc != M3D_OK) {   // step 4
        *n_sample = 0;
        return rc;
    }
    if (!dense) return M3D_OK;
    // step 5
    if (const int rc = m3d_voxel_down_sample(pts.data(), nrm.data(), nullptr, k, dist_step_dense, device, dense_xyz, dense_normals, nullptr,
                                             nullptr, nullptr, n_dense, nullptr);
        rc != M3D_OK) {
        *n_dense = 0;
        return rc;
    }
    return m3d_detect_boundary_points(dense_xyz, dense_normals, *n_dense, 2, radius, pts_num, 90.0, device, edge_indices, n_edges);
}
