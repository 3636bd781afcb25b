// m3d_generalfit_fp.hpp -- the host arithmetic of GeneralFit (include/misc3d/common/ransac.h:164-213, 296-330): from the
// moment sums of the inliers to the refined plane / sphere.  Plain C++, no HIP: the library (m3d_refine.cpp, m3d_fit.cpp)
// and the stand-alone check tests/cpp/test_generalfit_fp.cpp compile the same text (build with -ffp-contract=off).
//
// Two kernels' sums end here:
//   fused    compact_count_k<KIND, true> / compact_write_k<.., SUMS> + the fold of their partials: RAW moments of s = p - c0
//            about a provisional centre c0 -> moments_about_mean -> the closed form
//   two-pass sum_xyz_k + sum_moments_k + general_fit_sums_finish: the mean and the CENTRED moments -> the closed form
// c0 comes from the hypothesis' sample (slots 4..6 of the parameter record, minimal_fit_k): the plane's first sample point,
// the centroid of the sphere's four.  A sample point is an inlier of its own minimal model, so |mean - c0| is at most the
// inliers' extent.
//
// ACCURACY (include/misc3d_amd.h, "Refined parameters"): with the sums of either path the parameters lie within
// max(M err(oracle), F) of the exact closed form / least-squares answer, tests/test_gpu_generalfit.py.
#pragma once
#include <cmath>
#include <utility>

namespace m3d {

// Raw moments about the provisional centre c0 -> mean and centred moments.
//   mo[0..2] sum s   mo[3..8] sum s s^T (xx,xy,xz,yy,yz,zz)   mo[9..11] sum s |s|^2 (sphere; unread for a plane's closed form)
// With s = p - c0, m = (sum s) / n, r = s - m, q = |r|^2:
//   sum r r^T = sum s s^T - n m m^T
//   sum q     = trace of that
//   sum r q   = sum s|s|^2 - 2 (sum s s^T) m + m (2 n |m|^2 - trace(sum s s^T))
// The subtractions cancel by (|m| / extent of the inliers)^2 resp. ^3: c0 must lie AMONG the inliers (it does: a sample
// point, or the centroid of some).  A c0 at a sphere's centre, one radius away from a cap of inliers, loses (R / extent)^3.
inline void moments_about_mean(const double* mo, const double c0[3], double n, double mean[3], double centred[10]) {
    const double m[3] = {mo[0] / n, mo[1] / n, mo[2] / n};
    for (int k = 0; k < 3; ++k) mean[k] = c0[k] + m[k];
    const double S[6] = {mo[3], mo[4], mo[5], mo[6], mo[7], mo[8]};   // xx xy xz yy yz zz
    centred[0] = S[0] - n * m[0] * m[0];
    centred[1] = S[1] - n * m[0] * m[1];
    centred[2] = S[2] - n * m[0] * m[2];
    centred[3] = S[3] - n * m[1] * m[1];
    centred[4] = S[4] - n * m[1] * m[2];
    centred[5] = S[5] - n * m[2] * m[2];
    const double trS = (S[0] + S[3]) + S[5];
    const double mm = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
    const double Sm[3] = {(S[0] * m[0] + S[1] * m[1]) + S[2] * m[2], (S[1] * m[0] + S[3] * m[1]) + S[4] * m[2],
                          (S[2] * m[0] + S[4] * m[1]) + S[5] * m[2]};
    const double f = 2.0 * n * mm - trS;
    for (int k = 0; k < 3; ++k) centred[6 + k] = (mo[9 + k] - 2.0 * Sm[k]) + m[k] * f;
    centred[9] = (centred[0] + centred[3]) + centred[5];
}

// PlaneEstimator::GeneralFit, ransac.h:190-211
inline bool plane_from_moments(const double* mean, const double* s, double* out) {
    const double xx = s[0], xy = s[1], xz = s[2], yy = s[3], yz = s[4], zz = s[5];
    const double det_x = yy * zz - yz * yz;
    const double det_y = xx * zz - xz * xz;
    const double det_z = xx * yy - xy * xy;
    double a, b, c;
    if (det_x > det_y && det_x > det_z) {
        a = det_x;
        b = xz * yz - xy * zz;
        c = xy * yz - xz * yy;
    } else if (det_y > det_z) {
        a = xz * yz - xy * zz;
        b = det_y;
        c = xy * xz - yz * xx;
    } else {
        a = xy * yz - xz * yy;
        b = xy * xz - yz * xx;
        c = det_z;
    }
    const double norm = std::sqrt((a * a + b * b) + c * c);
    if (norm < 1.0e-8) return false;
    a /= norm;
    b /= norm;
    c /= norm;
    out[0] = a;
    out[1] = b;
    out[2] = c;
    out[3] = -((a * mean[0] + b * mean[1]) + c * mean[2]);
    return true;
}

// SphereEstimator::GeneralFit, ransac.h:296-330: least squares of [2x 2y 2z 1] w = x^2+y^2+z^2.
// The reference's bdcSvd(FullU) needs an N_inl x N_inl matrix (its own TODO, ransac.h:318-319);
// here the same least-squares problem is solved from the CENTRED normal equations
//   4 S c' = 2 sum(p' q),  w3' = sum(q)/n,  q = |p'|^2,  p' = p - mean,
// then centre = mean + c', r = sqrt(|c'|^2 + w3').  Same minimiser, parameters agree to ~1e-12.
inline bool sphere_from_moments(const double* mean, const double* s, double n, double* out) {
    double A[3][4] = {{4 * s[0], 4 * s[1], 4 * s[2], 2 * s[6]},
                      {4 * s[1], 4 * s[3], 4 * s[4], 2 * s[7]},
                      {4 * s[2], 4 * s[4], 4 * s[5], 2 * s[8]}};
    for (int col = 0; col < 3; ++col) {  // Gaussian elimination, partial pivoting
        int piv = col;
        for (int r = col + 1; r < 3; ++r)
            if (std::fabs(A[r][col]) > std::fabs(A[piv][col])) piv = r;
        if (piv != col)
            for (int k = 0; k < 4; ++k) std::swap(A[piv][k], A[col][k]);
        if (A[col][col] == 0.0) continue;
        for (int r = col + 1; r < 3; ++r) {
            const double f = A[r][col] / A[col][col];
            for (int k = col; k < 4; ++k) A[r][k] -= f * A[col][k];
        }
    }
    double c[3];
    for (int r = 2; r >= 0; --r) {
        double acc = A[r][3];
        for (int k = r + 1; k < 3; ++k) acc -= A[r][k] * c[k];
        c[r] = A[r][r] != 0.0 ? acc / A[r][r] : 0.0;
    }
    const double w3 = s[9] / n;
    out[0] = mean[0] + c[0];
    out[1] = mean[1] + c[1];
    out[2] = mean[2] + c[2];
    out[3] = std::sqrt(((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) + w3);
    return true;
}

}  // namespace m3d
