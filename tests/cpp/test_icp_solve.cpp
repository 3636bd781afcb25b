// test_icp_solve.cpp -- host-side check of point-to-plane ICP's 6 x 6 solve (misc3d_amd/csrc/m3d_icp_fp.hpp: the text the library
// compiles): no GPU, no library.  The identity for an empty or singular system and for a NaN input, a case worked out by
// hand, the rotation order of TransformVector6dToMatrix4d, the determinant's sign under row swaps, and the pivoted LDL^T
// against the residual on random positive definite systems.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "../../misc3d_amd/csrc/m3d_icp_fp.hpp"

using namespace m3d;

static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                               \
        }                                                             \
    } while (0)

static bool is_identity(const double* T) {
    for (int k = 0; k < 16; ++k)
        if (T[k] != ((k % 5 == 0) ? 1.0 : 0.0)) return false;
    return true;
}

// the record of m3d_icp_fp.hpp from a full symmetric matrix and a right-hand side
static void record(double count, const double A[36], const double jtr[6], double* sums) {
    for (int k = 0; k < kIcpPlaneSums; ++k) sums[k] = 0.0;
    sums[0] = count;
    int t = kIcpJtj;
    for (int r = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c) sums[t++] = A[6 * r + c];
    for (int k = 0; k < 6; ++k) sums[kIcpJtr + k] = jtr[k];
}

static double near(double a, double b) { return std::fabs(a - b); }

int main() {
    double sums[kIcpPlaneSums], U[16], A[36], b[6];
    // ---- an empty correspondence set: the identity, whatever the sums hold
    for (int k = 0; k < 36; ++k) A[k] = (k % 7 == 0) ? 3.0 : 0.0;
    for (int k = 0; k < 6; ++k) b[k] = 1.0;
    record(0.0, A, b, sums);
    CHECK(!icp_plane_update(sums, U) && is_identity(U));
    // ---- singular systems: all zeros; rank one (every J the same); |det| just below 1e-6
    for (int k = 0; k < 36; ++k) A[k] = 0.0;
    record(5.0, A, b, sums);
    CHECK(!icp_plane_update(sums, U) && is_identity(U));
    const double J[6] = {0.1, -0.2, 0.3, 0.5, 0.5, 0.7};
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) A[6 * r + c] = 7.0 * J[r] * J[c];
    record(7.0, A, b, sums);
    CHECK(!icp_plane_update(sums, U) && is_identity(U));
    for (int k = 0; k < 36; ++k) A[k] = (k % 7 == 0) ? 0.1 : 0.0;   // det = 1e-6 as rounded: 0.1^6 < 1e-6 in fp64?
    record(6.0, A, b, sums);
    {
        const double det = icp_det6(A);
        CHECK(icp_plane_update(sums, U) == !(std::fabs(det) < 1e-6));
        A[0] = 0.09;   // clearly below
        record(6.0, A, b, sums);
        CHECK(!icp_plane_update(sums, U) && is_identity(U));
    }
    // ---- a NaN anywhere in JTJ: the identity
    for (int k = 0; k < 36; ++k) A[k] = (k % 7 == 0) ? 3.0 : 0.0;
    A[6 * 2 + 4] = A[6 * 4 + 2] = std::numeric_limits<double>::quiet_NaN();
    record(9.0, A, b, sums);
    CHECK(!icp_plane_update(sums, U) && is_identity(U));
    A[6 * 2 + 4] = A[6 * 4 + 2] = std::numeric_limits<double>::infinity();
    record(9.0, A, b, sums);
    CHECK(!icp_plane_update(sums, U) && is_identity(U));
    // ---- by hand: JTJ = [[2, 1], [1, 2]] (+) diag(4, 8, 10, 16), JTr = -(0.3, 0, 0.2, 8, -5, 4)
    //      x0, x1 = (1 / 3) [[2, -1], [-1, 2]] (0.3, 0) = (0.2, -0.1); x2 = 0.05, x3 = 1, x4 = -0.5, x5 = 0.25
    for (int k = 0; k < 36; ++k) A[k] = 0.0;
    A[0] = 2.0, A[1] = 1.0, A[6] = 1.0, A[7] = 2.0, A[14] = 4.0, A[21] = 8.0, A[28] = 10.0, A[35] = 16.0;
    const double jtr[6] = {-0.3, 0.0, -0.2, -8.0, 5.0, -4.0};
    record(100.0, A, jtr, sums);
    CHECK(near(icp_det6(A), 3.0 * 4.0 * 8.0 * 10.0 * 16.0) < 1e-9);
    CHECK(icp_plane_update(sums, U));
    {
        const double x0 = 0.2, x1 = -0.1, x2 = 0.05;
        const double c0 = std::cos(x0), s0 = std::sin(x0), c1 = std::cos(x1), s1 = std::sin(x1), c2 = std::cos(x2), s2 = std::sin(x2);
        const double R[9] = {c2 * c1, c2 * s1 * s0 - s2 * c0, c2 * s1 * c0 + s2 * s0, s2 * c1, s2 * s1 * s0 + c2 * c0,
                             s2 * s1 * c0 - c2 * s0, -s1, c1 * s0, c1 * c0};
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) CHECK(near(U[4 * r + c], R[3 * r + c]) < 1e-14);
        CHECK(near(U[3], 1.0) < 1e-14 && near(U[7], -0.5) < 1e-14 && near(U[11], 0.25) < 1e-14);
        CHECK(U[12] == 0.0 && U[13] == 0.0 && U[14] == 0.0 && U[15] == 1.0);
    }
    // ---- the rotation order: Rz(90 deg) Rx(90 deg) takes e_x to e_y and e_y to e_z (Rx Rz would take e_x to e_z)
    {
        const double half_pi = std::acos(0.0);
        const double x[6] = {half_pi, 0.0, half_pi, 0.0, 0.0, 0.0};
        icp_vector6_to_matrix4(x, U);
        CHECK(near(U[0], 0.0) < 1e-15 && near(U[4], 1.0) < 1e-15 && near(U[8], 0.0) < 1e-15);    // column 0 = e_y
        CHECK(near(U[1], 0.0) < 1e-15 && near(U[5], 0.0) < 1e-15 && near(U[9], 1.0) < 1e-15);    // column 1 = e_z
        const double y[6] = {0.0, half_pi, 0.0, 0.0, 0.0, 0.0};   // Ry(90 deg): e_z -> e_x, e_x -> -e_z
        icp_vector6_to_matrix4(y, U);
        CHECK(near(U[2], 1.0) < 1e-15 && near(U[8], -1.0) < 1e-15);
    }
    // ---- the determinant changes sign with a row swap and equals the product of a triangular matrix's diagonal
    for (int k = 0; k < 36; ++k) A[k] = 0.0;
    for (int r = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c) A[6 * r + c] = (r == c) ? (double)(r + 2) : 0.25 * (double)(r + c);
    CHECK(near(icp_det6(A), 2.0 * 3.0 * 4.0 * 5.0 * 6.0 * 7.0) < 1e-9);
    for (int c = 0; c < 6; ++c) {
        const double t = A[c];
        A[c] = A[6 * 3 + c];
        A[6 * 3 + c] = t;
    }
    CHECK(near(icp_det6(A), -2.0 * 3.0 * 4.0 * 5.0 * 6.0 * 7.0) < 1e-9);
    // ---- the pivoted LDL^T against the residual on positive definite systems (B^T B + I: what JTJ is)
    std::srand(7);
    auto rnd = [] { return (double)std::rand() / RAND_MAX * 2.0 - 1.0; };
    for (int trial = 0; trial < 2000; ++trial) {
        double B[36], x[6];
        for (int k = 0; k < 36; ++k) B[k] = rnd();
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) {
                double v = (r == c) ? 1.0 : 0.0;
                for (int k = 0; k < 6; ++k) v += B[6 * k + r] * B[6 * k + c];
                A[6 * r + c] = v;
            }
        for (int k = 0; k < 6; ++k) b[k] = rnd();
        icp_ldlt_solve6(A, b, x);
        double res = 0.0;
        for (int r = 0; r < 6; ++r) {
            double v = -b[r];
            for (int c = 0; c < 6; ++c) v += A[6 * r + c] * x[c];
            res = std::fmax(res, std::fabs(v));
        }
        CHECK(res < 1e-12);
    }
    if (failures) {
        std::printf("FAILED: %d checks\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
