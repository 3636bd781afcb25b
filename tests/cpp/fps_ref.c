/* fps_ref.c -- plain-C restatement of misc3d::preprocessing::FarthestPointSampling's contract (the test oracle of
 * tests/test_preprocessing.py and tests/test_gpu_fps.py), written from the contract, not from the reference's source:
 *   dist[j] = +inf, farthest = 0; for each of S steps: emit farthest, s = p[farthest], best = 0; for j ascending:
 *   d = sum3 of the three rounded squares of the rounded differences, dist[j] = d < dist[j] ? d : dist[j],
 *   and dist[j] > best makes j the next farthest.
 * ORDER (as M3D_FP_ORDER): 0 and 2 = (e0 + e1) + e2, 1 = e0 + (e1 + e2).  Build with -ffp-contract=off.
 * fps_ref(xyz, n, S, out, dist_scratch): 1 <= S <= n, dist_scratch: n doubles.  The early cases stay with the callers. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifndef ORDER
#define ORDER 0
#endif

static double sum3(double e0, double e1, double e2) {
#if ORDER == 1
    return e0 + (e1 + e2);
#else
    return (e0 + e1) + e2;
#endif
}

int fps_ref_order(void) { return ORDER; }

void fps_ref(const double* xyz, size_t n, size_t S, uint64_t* out, double* dist) {
    size_t farthest = 0;
    for (size_t j = 0; j < n; ++j) dist[j] = INFINITY;
    for (size_t i = 0; i < S; ++i) {
        out[i] = farthest;
        const double sx = xyz[3 * farthest], sy = xyz[3 * farthest + 1], sz = xyz[3 * farthest + 2];
        double best = 0.0;
        for (size_t j = 0; j < n; ++j) {
            const double dx = xyz[3 * j] - sx, dy = xyz[3 * j + 1] - sy, dz = xyz[3 * j + 2] - sz;
            const double d = sum3(dx * dx, dy * dy, dz * dz);
            if (d < dist[j]) dist[j] = d;
            if (dist[j] > best) {
                best = dist[j];
                farthest = j;
            }
        }
    }
}
