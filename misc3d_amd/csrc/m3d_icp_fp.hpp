// m3d_icp_fp.hpp -- the host arithmetic of the RegistrationICP loop (icp_loop, m3d_registration.cpp): the compose step every
// estimator shares (icp_compose4), and ComputeTransformation of the estimators that reduce an iteration to a record
// (m3d_registration_icp_plane[_l1], m3d_registration_icp_colored: the rows of icp_iter_k): from the 30 sums to the 4 x 4 update; and the 3 x 3 solve of the
// colour gradient.  Plain C++, no HIP: the library and the stand-alone check tests/cpp/test_icp_solve.cpp compile the same text
// (build with -ffp-contract=off).
//
// [RECALL] Open3D 0.15.1 TransformationEstimationPointToPlane::ComputeTransformation ->
// SolveJacobianSystemAndObtainExtrinsicMatrix(JTJ, JTr) -> SolveLinearSystemPSD(JTJ, -JTr, check_det = true) ->
// TransformVector6dToMatrix4d; the numbered rules are in include/misc3d_amd.h (m3d_registration_icp_plane).
//
// The record of an iteration (kIcpPlaneSums doubles, summed per workgroup by icp_iter_k and written by icp_plane_final_k):
//   [0] correspondences   [1] sum d^2   [2 .. 22] JTJ, upper triangle by rows ((0,0) (0,1) .. (0,5) (1,1) .. (5,5))
//   [23 .. 28] JTr        [29] sum r^2
#pragma once
#include <cmath>
#include <cstring>

#if defined(__HIPCC__)
#define M3D_ICP_HD __host__ __device__
#else
#define M3D_ICP_HD
#endif

namespace m3d {

constexpr int kIcpPlaneSums = 30;
constexpr int kIcpJtj = 2, kIcpJtr = 23, kIcpR2 = 29;   // offsets into the record

// A.determinant() of a dynamic Eigen matrix: partial-pivot LU (row swaps flip the sign), the product of the pivots.
// A: 6 x 6 row-major.  A NaN entry gives NaN.
inline double icp_det6(const double* A) {
    double M[36];
    std::memcpy(M, A, sizeof(M));
    double det = 1.0;
    for (int k = 0; k < 6; ++k) {
        int p = k;
        double best = std::fabs(M[6 * k + k]);
        for (int i = k + 1; i < 6; ++i) {
            const double v = std::fabs(M[6 * i + k]);
            if (v > best) {
                best = v;
                p = i;
            }
        }
        if (p != k) {
            for (int j = 0; j < 6; ++j) {
                const double t = M[6 * k + j];
                M[6 * k + j] = M[6 * p + j];
                M[6 * p + j] = t;
            }
            det = -det;
        }
        const double piv = M[6 * k + k];
        det *= piv;
        if (piv == 0.0) return det * 0.0;   // (0, or NaN when det already is)
        for (int i = k + 1; i < 6; ++i) {
            const double f = M[6 * i + k] / piv;
            for (int j = k + 1; j < 6; ++j) M[6 * i + j] -= f * M[6 * k + j];
        }
    }
    return det;
}

// x = A.ldlt().solve(b) for a symmetric N x N A: P A P^T = L D L^T with the largest remaining |diagonal| as the pivot of
// every step (Eigen's LDLT), then the two triangular solves; a zero pivot's component of the solution is 0, as Eigen's.
// One text for both sizes: 6 (the pose, on the host) and 3 (the colour gradient, in color_gradient_k and on the host).
template <int N>
M3D_ICP_HD inline void icp_ldlt_solve(const double* A, const double* b, double* x) {
    double M[N * N];   // below the diagonal: L, column by column as the steps finish; the rest: what is left to factor
    for (int k = 0; k < N * N; ++k) M[k] = A[k];
    int perm[N];
    double D[N];
    for (int k = 0; k < N; ++k) perm[k] = k;
    for (int k = 0; k < N; ++k) {
        int p = k;
        double best = std::fabs(M[N * k + k]);
        for (int i = k + 1; i < N; ++i) {
            const double v = std::fabs(M[N * i + i]);
            if (v > best) {
                best = v;
                p = i;
            }
        }
        for (int q = k + 1; q < N; ++q) {   // (q == p found by a loop over constants: on the device M stays in registers)
            if (q != p) continue;
            for (int j = 0; j < N; ++j) {   // rows k, p (the finished columns of L with them)
                const double t = M[N * k + j];
                M[N * k + j] = M[N * q + j];
                M[N * q + j] = t;
            }
            for (int i = 0; i < N; ++i) {   // columns k, p
                const double t = M[N * i + k];
                M[N * i + k] = M[N * i + q];
                M[N * i + q] = t;
            }
            const int t = perm[k];
            perm[k] = perm[q];
            perm[q] = t;
        }
        const double d = M[N * k + k];
        D[k] = d;
        for (int i = k + 1; i < N; ++i) {
            const double l = d != 0.0 ? M[N * i + k] / d : 0.0;
            for (int j = k + 1; j < N; ++j) M[N * i + j] -= l * M[N * k + j];
            M[N * i + k] = l;
        }
    }
    double y[N];
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j)
            if (perm[i] == j) y[i] = b[j];
    for (int i = 0; i < N; ++i)   // L z = y
        for (int j = 0; j < i; ++j) y[i] -= M[N * i + j] * y[j];
    for (int i = 0; i < N; ++i) y[i] = D[i] != 0.0 ? y[i] / D[i] : 0.0;
    for (int i = N - 1; i >= 0; --i)   // L^T v = w
        for (int j = i + 1; j < N; ++j) y[i] -= M[N * j + i] * y[j];
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j)
            if (perm[i] == j) x[j] = y[i];
}
inline void icp_ldlt_solve6(const double* A, const double* b, double* x) { icp_ldlt_solve<6>(A, b, x); }
// the colour gradient's solve (rule G7 of m3d_color_gradient): no determinant check, the result stored as it comes
M3D_ICP_HD inline void icp_ldlt_solve3(const double* A, const double* b, double* x) { icp_ldlt_solve<3>(A, b, x); }

inline void icp_identity4(double* T) {
    for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

// transformation = update * transformation of the RegistrationICP loop: T = U T, 4 x 4 row-major, every entry associated as
// ((U0 T0 + U1 T4) + U2 T8) + U3 T12
inline void icp_compose4(const double* U, double* T) {
    double Tn[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            Tn[4 * r + c] = ((U[4 * r] * T[c] + U[4 * r + 1] * T[4 + c]) + U[4 * r + 2] * T[8 + c]) + U[4 * r + 3] * T[12 + c];
    std::memcpy(T, Tn, sizeof(Tn));
}

// TransformVector6dToMatrix4d: rotation Rz(x[2]) Ry(x[1]) Rx(x[0]), translation (x[3], x[4], x[5]).  T: 4 x 4 row-major.
inline void icp_vector6_to_matrix4(const double* x, double* T) {
    const double c0 = std::cos(x[0]), s0 = std::sin(x[0]), c1 = std::cos(x[1]), s1 = std::sin(x[1]), c2 = std::cos(x[2]),
                 s2 = std::sin(x[2]);
    icp_identity4(T);
    T[0] = c2 * c1;
    T[1] = (c2 * s1) * s0 - s2 * c0;
    T[2] = (c2 * s1) * c0 + s2 * s0;
    T[4] = s2 * c1;
    T[5] = (s2 * s1) * s0 + c2 * c0;
    T[6] = (s2 * s1) * c0 - c2 * s0;
    T[8] = -s1;
    T[9] = c1 * s0;
    T[10] = c1 * c0;
    T[3] = x[3];
    T[7] = x[4];
    T[11] = x[5];
}

// ComputeTransformation from an iteration's record: the identity for an empty correspondence set and when det(JTJ) is
// not finite or |det| < 1e-6 (SolveLinearSystemPSD's check); else x = LDLT(JTJ).solve(-JTr) turned into a matrix.
// Returns whether the system was solved.
inline bool icp_plane_update(const double* sums, double* U) {
    icp_identity4(U);
    if (!(sums[0] > 0.0)) return false;
    double A[36], b[6], x[6];
    int t = kIcpJtj;
    for (int r = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c) {
            A[6 * r + c] = sums[t];
            A[6 * c + r] = sums[t];
            ++t;
        }
    for (int k = 0; k < 6; ++k) b[k] = -sums[kIcpJtr + k];
    const double det = icp_det6(A);
    if (!std::isfinite(det) || std::fabs(det) < 1e-6) return false;
    icp_ldlt_solve6(A, b, x);
    icp_vector6_to_matrix4(x, U);
    return true;
}

}  // namespace m3d
