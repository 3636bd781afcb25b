// Host-side check of the pruned farthest point sampling's tile bound (misc3d_amd/csrc/m3d_fps_fp.hpp: fps_box_lb, the code
// fps_step_k runs): no GPU, no library.  Random (box, point of the box, selected point) triples over magnitudes 1e-3 ..
// 1e150 -- points inside the box and on its faces and corners, selected points inside, beside and far from it, signed
// zeros, squares that overflow -- and for every triple the bound must be <= the point's computed distance (both +inf
// counts as <=).  Prints "triples=N violations=V"; exit status 1 on a violation.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../misc3d_amd/csrc/m3d_fps_fp.hpp"

using namespace m3d;

int main(int argc, char** argv) {
    const long long trials = argc > 1 ? std::atoll(argv[1]) : 1000000;
    std::mt19937_64 rng(20261016);
    std::uniform_real_distribution<double> U01(0.0, 1.0);
    long long violations = 0, checked = 0;
    for (long long t = 0; t < trials; ++t) {
        const double mag = std::pow(10.0, -3.0 + 153.0 * U01(rng));   // 1e-3 .. 1e150 (and beyond through the offsets)
        double lo[3], hi[3], p[3], s[3];
        for (int k = 0; k < 3; ++k) {
            const double c = (U01(rng) - 0.5) * mag * (rng() % 4 == 0 ? 1e6 : 1.0);
            const double h = U01(rng) * mag * (rng() % 8 == 0 ? 0.0 : 1.0);
            lo[k] = c - h;
            hi[k] = c + h;
            if (lo[k] > hi[k]) std::swap(lo[k], hi[k]);
            switch (rng() % 6) {   // the point: inside, on a face, signed zero on a zero-width box
                case 0: p[k] = lo[k]; break;
                case 1: p[k] = hi[k]; break;
                default: p[k] = lo[k] + (hi[k] - lo[k]) * U01(rng); break;
            }
            if (p[k] < lo[k]) p[k] = lo[k];   // (the interpolation can round out of the box)
            if (p[k] > hi[k]) p[k] = hi[k];
            if (rng() % 64 == 0) lo[k] = hi[k] = p[k] = (rng() % 2 ? -0.0 : 0.0);
            switch (rng() % 5) {   // the selected point: inside the box, just outside, far away, on a face
                case 0: s[k] = lo[k] + (hi[k] - lo[k]) * U01(rng); break;
                case 1: s[k] = lo[k] - mag * 1e-9 * U01(rng); break;
                case 2: s[k] = hi[k] + mag * std::pow(10.0, 6.0 * U01(rng)) * U01(rng); break;
                case 3: s[k] = (rng() % 2 ? lo[k] : hi[k]); break;
                default: s[k] = (U01(rng) - 0.5) * mag * 4.0; break;
            }
            if (rng() % 128 == 0) s[k] = (rng() % 2 ? -0.0 : 0.0);
        }
        const double L = fps_box_lb(lo, hi, s[0], s[1], s[2]);
        const double d = fps_point_d(p[0], p[1], p[2], s[0], s[1], s[2]);
        ++checked;
        if (!(L <= d)) {
            if (violations < 5)
                std::printf("violation: L=%.17g d=%.17g p=(%.17g %.17g %.17g) s=(%.17g %.17g %.17g)\n", L, d, p[0], p[1], p[2],
                            s[0], s[1], s[2]);
            ++violations;
        }
    }
    std::printf("triples=%lld violations=%lld\n", checked, violations);
    return violations ? 1 : 0;
}
