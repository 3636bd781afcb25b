// Host-side pin of the grid arithmetic every cell-sorted grid is built from (misc3d_amd/csrc/m3d_grid_geom.hpp): no GPU, no
// library.  radius_grid_geom (registration's target grid, boundary detection, ProximityExtractor) against rows worked out by
// hand from its definition -- K, h, the dimensions and the origin compared with ==: results downstream are bit-exact only
// while the order of the operations stays -- an extent no finite cell holds (it must return, not spin), and sort_grid_bits /
// sort_grid_inv_h of the Hilbert sorts at their steps.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../misc3d_amd/csrc/m3d_grid_geom.hpp"

using namespace m3d;

static int bad = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            ++bad;                                                   \
            printf("FAILED line %d: %s\n", __LINE__, #cond);         \
        }                                                            \
    } while (0)

struct Row {
    double lo[3], hi[3], edge;
    int K0, K;
    double h;
    uint64_t dims[3];
};

int main() {
    const Row rows[] = {
        {{0, 0, 0}, {1, 2, 3}, 0.5, 4, 4, 0.125125, {26, 34, 42}},
        {{0, 0, 0}, {1, 2, 3}, 0.5, 1, 1, 0.5005, {8, 10, 12}},
        // K halved twice, h doubled four times: 506^3 = 129 554 216 cells <= 2^27
        {{0, 0, 0}, {1000, 1000, 1000}, 0.5, 4, 1, 2.002, {506, 506, 506}},
        {{-1, -1, -1}, {-1, -1, -1}, 0.25, 1, 1, 0.25025, {7, 7, 7}},   // a single point
    };
    for (const Row& r : rows) {
        const RadiusGridGeom g = radius_grid_geom(r.lo, r.hi, r.edge, r.K0);
        printf("edge %g K0 %d: K %d h %.17g dims %llu %llu %llu origin %.17g %.17g %.17g\n", r.edge, r.K0, g.K, g.h,
               (unsigned long long)g.dims[0], (unsigned long long)g.dims[1], (unsigned long long)g.dims[2], g.origin[0],
               g.origin[1], g.origin[2]);
        CHECK(g.K == r.K);
        CHECK(g.h == r.h);
        CHECK(1.0 / g.h == 1.0 / r.h);
        for (int k = 0; k < 3; ++k) {
            CHECK(g.dims[k] == r.dims[k]);
            CHECK(g.origin[k] == r.lo[k] - (2 * r.K + 1) * r.h);
        }
    }
    CHECK((uint64_t)506 * 506 * 506 <= ((uint64_t)1 << 27));
    {   // an extent that overflows (hi - lo = inf) drives h to infinity: returns with a non-finite h (proximity's error,
        // registration's one-cell grid) instead of spinning on inf / inf
        const double lo[3] = {-1e308, 0, 0}, hi[3] = {1e308, 1, 1};
        const RadiusGridGeom g = radius_grid_geom(lo, hi, 1.0, 4);
        CHECK(!std::isfinite(g.h));
        CHECK(g.K == 1);
        for (int k = 0; k < 3; ++k) CHECK(g.dims[k] == 7);
    }
    {   // the largest finite extents still end at a finite cell: the first doubling of h at which the table fits
        const double lo[3] = {0, 0, 0}, hi[3] = {1e308, 1, 1};
        const RadiusGridGeom g = radius_grid_geom(lo, hi, 1e-300, 4);
        CHECK(std::isfinite(g.h) && g.K == 1);
        CHECK(g.dims[0] == (uint64_t)(1e308 / g.h) + 7 && g.dims[1] == 7 && g.dims[2] == 7);
        CHECK(g.dims[0] * 49 <= ((uint64_t)1 << 27) && ((uint64_t)(1e308 / (0.5 * g.h)) + 7) * 49 > ((uint64_t)1 << 27));
    }
    {   // an infinite edge: one cell + pads at K0, at once
        const double lo[3] = {0, 0, 0}, hi[3] = {1, 2, 3};
        const RadiusGridGeom g = radius_grid_geom(lo, hi, INFINITY, 4);
        CHECK(g.K == 4 && std::isinf(g.h));
        for (int k = 0; k < 3; ++k) CHECK(g.dims[k] == 19);
    }

    const struct {
        uint64_t n;
        uint32_t bits;
    } steps[] = {{1, 1},    {64, 1},   {65, 2},      {512, 2},           {513, 3},
                 {4096, 3}, {4097, 4}, {1000000, 6}, {((uint64_t)1 << 27) + 1, 8}, {((uint64_t)1 << 31) - 1, 8}};
    for (const auto& s : steps) {
        printf("sort_grid_bits(%llu) = %u\n", (unsigned long long)s.n, sort_grid_bits(s.n));
        CHECK(sort_grid_bits(s.n) == s.bits);
    }
    CHECK(sort_grid_inv_h(0.0, 3) == 0.0);
    CHECK(sort_grid_inv_h(-1.0, 3) == 0.0);
    CHECK(sort_grid_inv_h(2.0, 3) == 8.0 / (2.0 * (1.0 + 1e-9)));
    CHECK(sort_grid_inv_h(0.3, 8) == 256.0 / (0.3 * (1.0 + 1e-9)));

    printf(bad ? "FAILED: %d checks\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
