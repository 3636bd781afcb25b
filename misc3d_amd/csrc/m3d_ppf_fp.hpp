// m3d_ppf_fp.hpp -- the arithmetic of the PPF table and vote (include/misc3d_amd.h, "PPF voting"): the ONE place the pair
// features, their bins, the alpha bin and the spread of a quantised feature exist.  Shared by the kernels (m3d_ppf.hip), the
// host driver (m3d_ppf.cpp) and a host check (tests/cpp/test_ppf_mirror.cpp); no dependency on M3D_FP_ORDER (every sum is
// written out).  Build with -ffp-contract=off; divisions and square roots are the correctly rounded fp64 ones of hipcc's
// defaults for gfx950 and of every x86-64 compiler.  No bin is decided by a transcendental function: the edges below are
// computed once on the host (ppf_make_tables) and compared against.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define M3D_PPF_HD __host__ __device__ __forceinline__
#else
#define M3D_PPF_HD inline
#endif

namespace m3d {

constexpr int kPpfMaxAlphaBins = 64;   // alpha_model_num: one bit of a 64-bit flag word each
constexpr int kPpfMaxAngleBins = 32;   // angle_num = (alpha_model_num + 1) / 2

struct PpfTables {
    int32_t angle_num, alpha_num, dist_num, spread_k;   // spread_k: 2 in faster mode, 3 otherwise
    double cos_edge[kPpfMaxAngleBins];     // [k] = cos((k + 1/2) step), k < angle_num - 1 (descending)
    double alpha_c[kPpfMaxAlphaBins];      // [b] = cos(theta_b), theta_b = (b + 1/2) step - pi, b < alpha_num - 1 (ascending angle)
    double alpha_s[kPpfMaxAlphaBins];      // [b] = sin(theta_b)
    const double* dist_edge2;              // [k] = ((k + 1/2) dist_step)^2, k < dist_num (ascending)
};

// round(acos(x) / step): the number of edges with acos(x) >= (k + 1/2) step, i.e. x <= cos_edge[k].  x > 1 gives 0 and
// x < -1 the end bin angle_num - 1 (the reference's acos is NaN there).
M3D_PPF_HD int ppf_angle_bin(const PpfTables& T, double x) {
    int b = 0;
    for (int k = 0; k < T.angle_num - 1; ++k) b += x <= T.cos_edge[k] ? 1 : 0;
    return b;
}

// round(sqrt(d2) / dist_step): the number of edges with d2 >= dist_edge2[k]; dist_num = beyond the table (the pair is skipped)
M3D_PPF_HD int ppf_dist_bin(const PpfTables& T, double d2) {
    int b = 0;
    for (int k = 0; k < T.dist_num; ++k) b += d2 >= T.dist_edge2[k] ? 1 : 0;
    return b;
}

// round((atan2(-z, y) + pi) / step): the number of edges theta_b <= alpha, alpha the angle of w = (y, -z) in [-pi, pi].  An edge
// e = (c, s) in the upper half plane (s > 0) is passed when w is in the upper half plane (-z has no sign bit) and
// c (-z) - s y >= 0; an edge in the lower half plane when w is in the upper one or c (-z) - s y >= 0.  -z = -0 with y < 0 is
// -pi (bin 0), -z = +0 with y < 0 is pi (the last bin), as atan2 has them; y == 0 and z == 0 counts as alpha = 0.
M3D_PPF_HD int ppf_alpha_bin(const PpfTables& T, double y, double z) {
    const double v = -z;
    if (y == 0.0 && v == 0.0) return T.angle_num - 1;
    const bool upper = !__builtin_signbit(v);
    int b = 0;
    for (int k = 0; k < T.alpha_num - 1; ++k) {
        const bool ccw = T.alpha_c[k] * v - T.alpha_s[k] * y >= 0.0;
        const bool pass = T.alpha_s[k] > 0.0 ? (upper && ccw) : (upper || ccw);
        b += pass ? 1 : 0;
    }
    return b;
}

// d2 of the pair, the library's neighbourhood sum
M3D_PPF_HD double ppf_d2(const double* p0, const double* p1) {
    const double dx = p1[0] - p0[0], dy = p1[1] - p0[1], dz = p1[2] - p0[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// The quantised feature q[0..3] (CalcPPF + QuantizePPF, ppf_estimation.cpp:642-661) and the alpha bin (CalcAlpha, :699-704,
// + round) of the pair (p0, n0) -> (p1, n1) under the frame of p0; frame = rows 1 and 2 of [R | t] (8 doubles).  false: the
// pair is skipped (d2 == 0, or a distance bin beyond the table -- which a non-finite d2 is).
M3D_PPF_HD bool ppf_pair_bins(const PpfTables& T, const double* p0, const double* n0, const double* p1, const double* n1,
                              const double* frame, int* q, int* qalpha) {
    const double dx = p1[0] - p0[0], dy = p1[1] - p0[1], dz = p1[2] - p0[2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (!(d2 > 0.0)) return false;
    q[3] = ppf_dist_bin(T, d2);
    if (q[3] >= T.dist_num) return false;
    const double norm = sqrt(d2);
    const double ux = dx / norm, uy = dy / norm, uz = dz / norm;
    q[0] = ppf_angle_bin(T, (n0[0] * ux + n0[1] * uy) + n0[2] * uz);
    q[1] = ppf_angle_bin(T, (n1[0] * ux + n1[1] * uy) + n1[2] * uz);
    q[2] = ppf_angle_bin(T, (n0[0] * n1[0] + n0[1] * n1[1]) + n0[2] * n1[2]);
    const double y = ((frame[0] * p1[0] + frame[1] * p1[1]) + frame[2] * p1[2]) + frame[3];
    const double z = ((frame[4] * p1[0] + frame[5] * p1[1]) + frame[6] * p1[2]) + frame[7];
    *qalpha = ppf_alpha_bin(T, y, z);
    return true;
}

// HashPPF (:663-666)
M3D_PPF_HD uint32_t ppf_cell(const PpfTables& T, const int* q) {
    const uint32_t a = (uint32_t)T.angle_num;
    return (uint32_t)q[0] + a * ((uint32_t)q[1] + a * ((uint32_t)q[2] + a * (uint32_t)q[3]));
}

// SpreadPPF (:706-743): the s-th cell of the loop nest (s0 over the distance, s1, s2, s3 over the angles; s < 3 k^3), or
// -1 where a shifted bin leaves its range
M3D_PPF_HD int ppf_spread_count(const PpfTables& T) { return 3 * T.spread_k * T.spread_k * T.spread_k; }
M3D_PPF_HD int64_t ppf_spread_cell(const PpfTables& T, const int* q, int s) {
    const int k = T.spread_k;
    const int s3 = s % k, s2 = (s / k) % k, s1 = (s / (k * k)) % k, s0 = s / (k * k * k);
    int t[4] = {q[0] + s1 - 1, q[1] + s2 - 1, q[2] + s3 - 1, q[3] + s0 - 1};
    if (t[3] < 0 || t[3] >= T.dist_num) return -1;
    for (int c = 0; c < 3; ++c)
        if (t[c] < 0 || t[c] >= T.angle_num) return -1;
    return (int64_t)ppf_cell(T, t);
}

// the accumulator column of a table entry under a scene alpha bin (alpha_lut_, :1259-1265)
M3D_PPF_HD int ppf_alpha_index(int quant_alpha, int quantize_alpha, int alpha_num) {
    return (quant_alpha - quantize_alpha + alpha_num) % alpha_num;
}

// the pair filter of the vote (:456-459): true = the neighbour is left out
M3D_PPF_HD bool ppf_pair_filtered(double d2, const double* n0, const double* n1, double dist_thresh, double cos_thresh) {
    return sqrt(d2) < dist_thresh && (n1[0] * n0[0] + n1[1] * n0[1]) + n1[2] * n0[2] > cos_thresh;
}

// ---- host only: the derived sizes (Train, :538-542) and the edge tables
struct PpfSizes {
    int64_t angle_num, alpha_num, dist_num, table_size;
    double dist_step;
};
inline PpfSizes ppf_sizes(double diameter, double rel_sample_dist, double angle_step) {
    PpfSizes s;
    const double a = std::round(M_PI / angle_step) + 1.0, d = std::round(1.0 / rel_sample_dist) + 1.0;
    const bool ok = a >= 1.0 && a <= 1e6 && d >= 1.0 && d <= 1e9;   // (false for NaN)
    s.angle_num = ok ? (int64_t)a : 0;
    s.dist_num = ok ? (int64_t)d : 0;
    s.alpha_num = 2 * s.angle_num - 1;
    s.table_size = s.angle_num * s.angle_num * s.angle_num * s.dist_num;
    s.dist_step = diameter * rel_sample_dist;
    return s;
}
// T's edges for sizes that passed the checks (alpha_num <= 64); T.dist_edge2 = edge2.data() (the caller re-points it at a
// device copy for the kernels)
inline void ppf_make_tables(const PpfSizes& s, double angle_step, bool faster_mode, PpfTables* T, std::vector<double>* edge2) {
    T->angle_num = (int32_t)s.angle_num;
    T->alpha_num = (int32_t)s.alpha_num;
    T->dist_num = (int32_t)s.dist_num;
    T->spread_k = faster_mode ? 2 : 3;
    for (int k = 0; k < kPpfMaxAngleBins; ++k) T->cos_edge[k] = k < s.angle_num - 1 ? std::cos(((double)k + 0.5) * angle_step) : -2.0;
    for (int b = 0; b < kPpfMaxAlphaBins; ++b) {
        const double th = ((double)b + 0.5) * angle_step - M_PI;
        const bool used = b < s.alpha_num - 1 && th <= M_PI;   // (an edge beyond pi is never passed: NaN compares false)
        T->alpha_c[b] = used ? std::cos(th) : std::nan("");
        T->alpha_s[b] = used ? std::sin(th) : 1.0;
    }
    edge2->resize((size_t)s.dist_num);
    for (int64_t k = 0; k < s.dist_num; ++k) {
        const double e = ((double)k + 0.5) * s.dist_step;
        (*edge2)[(size_t)k] = e * e;
    }
    T->dist_edge2 = edge2->data();
}

}  // namespace m3d
