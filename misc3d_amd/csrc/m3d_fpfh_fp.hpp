// m3d_fpfh_fp.hpp -- the arithmetic of the FPFH descriptor (include/misc3d_amd.h, "FPFH"), shared by the kernels
// (m3d_fpfh.hip) and the host check m3d_bench_fpfh_pair_bins.  [RECALL] of Open3D 0.15.1's ComputePairFeatures /
// ComputeSPFHFeature / ComputeFPFHFeature (pipelines/registration/Feature.cpp); the header's text is the contract.
#pragma once
#include "m3d_eig3.hpp"
#include "m3d_fp.hpp"

namespace m3d {

constexpr int kFpfhBins = 11;    // bins per feature
constexpr int kFpfhDim = 33;     // three features
constexpr int kFpfhMaxNn = 128;  // longest neighbour list (the k-NN grid path's cap)

// The contract's `acos(|a1|) > acos(|a2|)` is the HOST libm's: two acos implementations that are each within a few ulp may
// order two nearly equal arguments differently (estimated normals of neighbouring points often come from the same
// neighbours and agree to an ulp).  kFpfhTieBand bounds, relative to the larger value, how far two acos results may be
// apart and still be ordered differently by another libm: 64 eps covers 16 ulp of error on each side.  Equal arguments
// are no tie (any acos gives them equal results), nor are NaN results (|a| > 1: NaN under every acos, comparison false).
constexpr double kFpfhTieBand = 64.0 * 2.220446049250313e-16;

// (f0, f1, f2) of (p1, n1) with the neighbour (p2, n2); all 0 when the points coincide or dp is parallel to the normal.
// *near_tie (may be null) is set when the swap decision falls inside kFpfhTieBand (never cleared).
M3D_HD void fpfh_pair_features(const double* p1, const double* n1, const double* p2, const double* n2, double* f,
                               bool* near_tie = nullptr) {
    f[0] = f[1] = f[2] = 0.0;
    double dx = p2[0] - p1[0], dy = p2[1] - p1[1], dz = p2[2] - p1[2];
    const double d = norm3(dx, dy, dz);
    if (d == 0.0) return;
    const double a1 = dot3(n1[0], n1[1], n1[2], dx, dy, dz) / d;
    const double a2 = dot3(n2[0], n2[1], n2[2], dx, dy, dz) / d;
    const double *na = n1, *nb = n2;
    double f2;
    const double x1 = fabs(a1), x2 = fabs(a2), y1 = acos(x1), y2 = acos(x2);
    if (near_tie && x1 != x2 && fabs(y1 - y2) <= kFpfhTieBand * fmax(y1, y2)) *near_tie = true;
    if (y1 > y2) {   // the frame goes on the normal that is closer to the line of the pair
        na = n2;
        nb = n1;
        dx = -dx;
        dy = -dy;
        dz = -dz;
        f2 = -a2;
    } else {
        f2 = a1;
    }
    double vx = dy * na[2] - dz * na[1];
    double vy = dz * na[0] - dx * na[2];
    double vz = dx * na[1] - dy * na[0];
    const double vn = norm3(vx, vy, vz);
    if (vn == 0.0) return;
    vx /= vn;
    vy /= vn;
    vz /= vn;
    const double wx = na[1] * vz - na[2] * vy;
    const double wy = na[2] * vx - na[0] * vz;
    const double wz = na[0] * vy - na[1] * vx;
    f[2] = f2;
    f[1] = dot3(vx, vy, vz, nb[0], nb[1], nb[2]);
    f[0] = atan2(dot3(wx, wy, wz, nb[0], nb[1], nb[2]), dot3(na[0], na[1], na[2], nb[0], nb[1], nb[2]));
}

// clamp(floor(x)) to [0, 10]; a NaN goes to 0
M3D_HD int fpfh_clamp_bin(double x) {
    if (!(x >= 0.0)) return 0;
    if (x >= 11.0) return kFpfhBins - 1;
    return (int)x;   // (truncation == floor for x >= 0)
}
// the three bins (columns of the 33-row) a pair adds to
M3D_HD void fpfh_bins(const double* f, int* b) {
    b[0] = fpfh_clamp_bin(11.0 * (f[0] + M_PI) / (2.0 * M_PI));
    b[1] = kFpfhBins + fpfh_clamp_bin(11.0 * (f[1] + 1.0) * 0.5);
    b[2] = 2 * kFpfhBins + fpfh_clamp_bin(11.0 * (f[2] + 1.0) * 0.5);
}
// the increment of one pair in the SPFH row of a point with m neighbours (itself included); 0 for m <= 1
M3D_HD double fpfh_incr(uint32_t m) { return m > 1 ? 100.0 / (double)(m - 1) : 0.0; }
// an SPFH entry from its pair count (every increment of a row is the same incr)
M3D_HD double fpfh_spfh_value(uint32_t count, double incr) { return (double)count * incr; }
// the weighted neighbour term: spfh / d2 (the SQUARED distance)
M3D_HD double fpfh_weighted(double spfh, double d2) { return spfh / d2; }
// out[j] from the accumulated neighbour terms acc[j], their group sum and the point's own SPFH entry
M3D_HD double fpfh_finish(double acc, double group_sum, double own) {
    const double s = group_sum != 0.0 ? 100.0 / group_sum : 0.0;
    return acc * s + own;
}

// the normal of m >= 3 neighbours from their raw sums s = (x, y, z, xx, xy, xz, yy, yz, zz), taken in list order:
// covariance in cumulant form (oracle/misc3d_oracle_boundary.c:87-112), eigenvector of the smallest eigenvalue (J3x3)
M3D_HD void fpfh_normal_from_sums(double* s, uint32_t m, double* n) {
    const double inv = 1.0 / (double)m;
    for (int t = 0; t < 9; ++t) s[t] *= inv;
    double Cm[9];
    Cm[0] = s[3] - s[0] * s[0];
    Cm[1] = s[4] - s[0] * s[1];
    Cm[2] = s[5] - s[0] * s[2];
    Cm[4] = s[6] - s[1] * s[1];
    Cm[5] = s[7] - s[1] * s[2];
    Cm[8] = s[8] - s[2] * s[2];
    Cm[3] = Cm[1];
    Cm[6] = Cm[2];
    Cm[7] = Cm[5];
    j3x3_smallest_eigvec(Cm, n);
    if (!((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2] > 0.0)) {   // zero length (or NaN): Open3D's fallback
        n[0] = 0.0;
        n[1] = 0.0;
        n[2] = 1.0;
    }
}
// OrientNormalsTowardsCameraLocation for one point
M3D_HD void fpfh_orient(const double* p, const double* cam, double* n) {
    const double vx = cam[0] - p[0], vy = cam[1] - p[1], vz = cam[2] - p[2];
    if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0) {
        const double l = norm3(vx, vy, vz);
        if (l == 0.0) {
            n[0] = 0.0;
            n[1] = 0.0;
            n[2] = 1.0;
        } else {
            n[0] = vx / l;
            n[1] = vy / l;
            n[2] = vz / l;
        }
    } else if (dot3(n[0], n[1], n[2], vx, vy, vz) < 0.0) {
        n[0] = -n[0];
        n[1] = -n[1];
        n[2] = -n[2];
    }
}

}  // namespace m3d
