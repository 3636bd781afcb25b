// m3d_fps_fp.hpp -- the arithmetic of farthest point sampling (m3d_fps.hip), shared by the device kernels and the host-side
// check tests/cpp/test_fps_bound.cpp (no GPU, no library: the same expressions compiled by g++).
//
// FarthestPointSampling (src/filter.cpp:13-52) keeps, for every point j, dist[j] = min over the selected points s of
// (p_j - s).squaredNorm(), a 3-element reduction: sum3 of the three rounded squares of the rounded differences (m3d_fp.hpp,
// so the order1 / order2 builds follow the FP-order switch).  std::min(dist, d) is `d < dist ? d : dist`: a NaN d never
// lowers a distance.
//
// The pruned path skips a tile of points for a step when a lower bound L of every point's COMPUTED d is >= the largest
// current distance of the tile (tmax): then d < dist[j] is false for all its points and the step changes nothing there.
// fps_box_lb is that bound for the tile's exact fp64 box [lo, hi]: per axis the gap fl(c - s) with c = clamp(s, lo, hi),
// squared and summed in the same association as fps_point_d.  Exact, with no margin:
//   * for every coordinate p of the box on that axis, |c - s| <= |p - s| with c - s and p - s of the same sign (or c - s = 0),
//     and IEEE subtraction is monotone, so |fl(c - s)| <= |fl(p - s)|;
//   * squaring and adding non-negative numbers under round-to-nearest are monotone as well,
// so L <= d for every point of the box -- overflow to +inf included.  A NaN in s makes L NaN and L >= tmax false: no skip.
#pragma once
#include "m3d_fp.hpp"

namespace m3d {

constexpr int kFpsTilePoints = 512;   // points per tile of the pruned path (one wave x 8 rows of 64)

// (p - s).squaredNorm() as the reference computes it
M3D_HD double fps_point_d(double px, double py, double pz, double sx, double sy, double sz) {
    const double dx = px - sx, dy = py - sy, dz = pz - sz;
    return sum3(dx * dx, dy * dy, dz * dz);
}
// one axis of the box bound: the rounded gap between s and the nearest coordinate of [lo, hi]
M3D_HD double fps_axis_gap(double s, double lo, double hi) {
    const double c = fmin(fmax(s, lo), hi);
    return c - s;
}
// lower bound of fps_point_d(p, s) over every p in the box lo[0..2] .. hi[0..2]
M3D_HD double fps_box_lb(const double* lo, const double* hi, double sx, double sy, double sz) {
    const double gx = fps_axis_gap(sx, lo[0], hi[0]), gy = fps_axis_gap(sy, lo[1], hi[1]),
                 gz = fps_axis_gap(sz, lo[2], hi[2]);
    return sum3(gx * gx, gy * gy, gz * gz);
}
// the argmax key of a step: larger distance first, then the lower ORIGINAL index (the reference's ascending scan with a
// strict `>` keeps the first index that reaches the maximum)
M3D_HD bool fps_better(double d1, uint32_t i1, double d2, uint32_t i2) { return d1 > d2 || (d1 == d2 && i1 < i2); }

}  // namespace m3d
