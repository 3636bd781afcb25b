// m3d_proximity_fp.hpp -- the arithmetic of ProximityExtractor's evaluators (m3d_proximity.hip), shared by the device kernels,
// the driver that derives the cut-offs (m3d_proximity.cpp) and the host check m3d_bench_proximity_cutoffs.
//
// The reference's evaluators see dist = sqrt(d2) and an angle acos(dot3(n_i, n_j)) (src/proximity_extraction.cpp,
// include/misc3d/segmentation/proximity_extraction.h).  The device calls neither sqrt nor acos: the host turns every
// threshold into exact cut-offs on the pre-sqrt / pre-acos quantity, found by bisection over the doubles, which needs
// nothing but the monotonicity of the correctly rounded sqrt and of the host's acos.
//   * d2_cut = the smallest double c >= 0 with sqrt(c) >= t (0 for t <= 0, +inf for t = +inf, NaN for t = NaN).  Then for
//     every d2 that is not NaN, sqrt(d2) >= t <=> d2 >= d2_cut; a NaN d2 or a NaN t fails both sides.  Hence
//       Distance:        dist < t           <=>  d2 < d2_cut
//       DistanceNormals: !(dist >= t)       <=>  !(d2 >= d2_cut)      (a NaN dist passes this half, as in the reference)
//   * the angle test accepts dot exactly on [lo1, hi1] u [lo2, hi2] (NaN fails both):
//       max_angle = deg / 180 * M_PI (Deg2Rad, utils.h:331-333) >= 0 (-0.0 included): acos(dot) <= max_angle, dot in
//         [c, 1] with c the smallest dot in [-1, 1] that passes (acos(1) = 0 always passes);
//       max_angle < 0: min(angle, M_PI - angle) <= -max_angle <=> angle <= m || M_PI - angle <= m (m = -max_angle): dot in
//         [c1, 1] u [-1, c2], c2 the largest dot whose M_PI - acos(dot) passes (acos(-1) = M_PI: -1 always passes);
//       max_angle NaN: nothing passes.
//     A dot outside [-1, 1] is NaN under acos and fails every comparison: the intervals never reach past +-1.
#pragma once
#include "m3d_fp.hpp"

#include <cmath>
#include <cstdint>
#include <cstring>

namespace m3d {

// evaluator kinds (the values of M3D_PROX_* in include/misc3d_amd.h)
constexpr int kProxDistance = 1, kProxNormals = 2, kProxDistanceNormals = 3;

struct ProxCut {
    int kind = 0;
    double d2_cut = 0.0;
    double lo1 = 1.0, hi1 = -1.0, lo2 = 1.0, hi2 = -1.0;   // empty intervals
};

// squared distance of the radius search (KDTreeFlann's L2 in the convention of detect_boundary_points' Radius mode)
M3D_HD double prox_d2(double dx, double dy, double dz) { return (dx * dx + dy * dy) + dz * dz; }
// radius membership: the one place where the unpinned `<=` lives
M3D_HD bool prox_in_radius(double d2, double r2) { return d2 <= r2; }
M3D_HD bool prox_dot_ok(const ProxCut& c, double dot) {
    return (dot >= c.lo1 && dot <= c.hi1) || (dot >= c.lo2 && dot <= c.hi2);
}
// evaluator(i, j, sqrt(d2)) of a built-in kind; dot = dot3(n_i, n_j) (not read for kProxDistance)
M3D_HD bool prox_accept(const ProxCut& c, double d2, double dot) {
    if (c.kind == kProxDistance) return d2 < c.d2_cut;
    if (c.kind == kProxDistanceNormals && d2 >= c.d2_cut) return false;
    return prox_dot_ok(c, dot);
}

// ---- host: the cut-offs ------------------------------------------------------------------------------------------------
// total order of the doubles as unsigned keys (-inf < ... < -0 < +0 < ... < +inf)
inline uint64_t prox_key(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
inline double prox_unkey(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double v;
    std::memcpy(&v, &u, 8);
    return v;
}
// smallest x in [lo, hi] with pred(x), given pred(hi) and pred monotone false -> true over the doubles
template <class P>
inline double prox_first_true(double lo, double hi, P pred) {
    if (pred(lo)) return lo;
    uint64_t a = prox_key(lo), b = prox_key(hi);   // pred(a) false, pred(b) true
    while (b - a > 1) {
        const uint64_t m = a + (b - a) / 2;
        if (pred(prox_unkey(m))) b = m;
        else a = m;
    }
    return prox_unkey(b);
}

inline double prox_d2_cut(double t) {
    if (std::isnan(t)) return NAN;
    if (t <= 0.0) return 0.0;
    if (std::isinf(t)) return INFINITY;
    return prox_first_true(0.0, INFINITY, [t](double c) { return std::sqrt(c) >= t; });
}

inline void prox_angle_cut(double angle_deg, ProxCut* c) {
    const double max_angle = angle_deg / 180 * M_PI;   // Deg2Rad
    c->lo1 = c->lo2 = 1.0;
    c->hi1 = c->hi2 = -1.0;
    if (std::isnan(max_angle)) return;
    const double m = max_angle >= 0.0 ? max_angle : -max_angle;
    c->lo1 = prox_first_true(-1.0, 1.0, [m](double d) { return std::acos(d) <= m; });
    c->hi1 = 1.0;
    if (max_angle >= 0.0) return;
    // the largest d with M_PI - acos(d) <= m: one below the first d where it fails (true -> false as d grows)
    auto fails = [m](double d) { return !(M_PI - std::acos(d) <= m); };
    c->lo2 = -1.0;
    c->hi2 = fails(1.0) ? prox_unkey(prox_key(prox_first_true(-1.0, 1.0, fails)) - 1) : 1.0;
}

inline ProxCut prox_cut(int kind, double dist, double angle_deg) {
    ProxCut c;
    c.kind = kind;
    c.d2_cut = prox_d2_cut(dist);
    if (kind != kProxDistance) prox_angle_cut(angle_deg, &c);
    return c;
}

}  // namespace m3d
