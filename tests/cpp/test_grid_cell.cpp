// Host-side pin of the cell lookup every cell-sorted grid shares (misc3d_amd/csrc/m3d_grid_cell.hpp): no GPU, no library.
//   1. grid_cell / grid_cell_frac against the expression the kernels carried before the header existed, restated literally
//      below: the return value, the three indices and the three fractions compared with == on a million random points per
//      descriptor (NaN and +-inf in every coordinate among them) and on points placed exactly on the cell faces around
//      lo_pad and n - lo_pad with their neighbouring doubles on both sides.
//   2. the padding contract of radius_grid_geom (m3d_grid_geom.hpp): every point of [lo, hi] has a cell with lo_pad = 0, every
//      query of [lo - edge, hi + edge] has one with lo_pad = K, and the x-rows row + (-K .. K + 1) of all (2K + 1)^2 rows of
//      its block stay inside [0, ncell], and the block covers the edge (a point one edge from the query along any diagonal
//      lies within K cells of it) -- for K kept, halved from a power of two and from 3, 5, 6, 7 and 12.  The lower margin is K + 1 - K / 1.001 cells, the upper just under one cell: far above
//      any rounding, so the check is exact.
//   3. grid_cell_id and grid_row_span on triples worked out by hand.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../misc3d_amd/csrc/m3d_grid_cell.hpp"
#include "../../misc3d_amd/csrc/m3d_grid_geom.hpp"

using namespace m3d;

static int bad = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            if (++bad <= 20) printf("FAILED line %d: %s\n", __LINE__, #cond); \
        }                                                            \
    } while (0)

struct Desc {   // what grid_cell reads of GridDesc (which carries device vector types and cannot be included here)
    double ox, oy, oz, inv_h;
    uint32_t nx, ny, nz;
    int K;
};

// the kernels' former cell_of_frac (= cell_of / cache_cell_of / prox_cell + the fractions), word for word
static bool parent_cell(const Desc& g, double x, double y, double z, int lo_pad, int* ix, int* iy, int* iz, double* frx,
                        double* fry, double* frz) {
    const double fx = (x - g.ox) * g.inv_h, fy = (y - g.oy) * g.inv_h, fz = (z - g.oz) * g.inv_h;
    if (!(fx >= (double)lo_pad && fx < (double)(g.nx - lo_pad) && fy >= (double)lo_pad &&
          fy < (double)(g.ny - lo_pad) && fz >= (double)lo_pad && fz < (double)(g.nz - lo_pad)))
        return false;
    *ix = (int)fx;
    *iy = (int)fy;
    *iz = (int)fz;
    *frx = fx - (double)*ix;
    *fry = fy - (double)*iy;
    *frz = fz - (double)*iz;
    return true;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double uni() { return (double)(rnd() >> 11) * 0x1p-53; }

static uint64_t n_in = 0, n_out = 0;
static void same_as_parent(const Desc& g, double x, double y, double z, int lo_pad) {
    const int s = 0x5A5A5A5A;
    int a[3] = {s, s, s}, b[3] = {s, s, s}, c[3] = {s, s, s};
    double fa[3] = {-7.0, -7.0, -7.0}, fb[3] = {-7.0, -7.0, -7.0};
    const bool ra = parent_cell(g, x, y, z, lo_pad, &a[0], &a[1], &a[2], &fa[0], &fa[1], &fa[2]);
    const bool rb = grid_cell_frac(g, x, y, z, lo_pad, &b[0], &b[1], &b[2], &fb[0], &fb[1], &fb[2]);
    const bool rc = grid_cell(g, x, y, z, lo_pad, &c[0], &c[1], &c[2]);
    CHECK(ra == rb && ra == rc);
    for (int k = 0; k < 3; ++k) {
        CHECK(a[k] == b[k] && a[k] == c[k]);   // (a rejected point leaves the sentinels in place on every side)
        CHECK(fa[k] == fb[k]);
        if (ra) CHECK(b[k] >= lo_pad && fb[k] >= 0.0 && fb[k] < 1.0);
    }
    (ra ? n_in : n_out)++;
}

static void compare(const Desc& g, const char* name) {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double h = 1.0 / g.inv_h;
    const double o[3] = {g.ox, g.oy, g.oz};
    const uint32_t n[3] = {g.nx, g.ny, g.nz};
    const int pads[2] = {0, g.K};
    const uint64_t in0 = n_in, out0 = n_out;
    for (int i = 0; i < 1000000; ++i) {   // two cells beyond the table on either side; one coordinate in 32 special
        double p[3];
        for (int k = 0; k < 3; ++k) {
            p[k] = o[k] + (uni() * ((double)n[k] + 4.0) - 2.0) * h;
            const uint64_t r = rnd() % 96u;
            if (r < 3) p[k] = r == 0 ? nan : (r == 1 ? inf : -inf);
        }
        for (int lo_pad : pads) same_as_parent(g, p[0], p[1], p[2], lo_pad);
    }
    for (int lo_pad : pads)   // on the faces: o + k / inv_h, k around lo_pad and n - lo_pad (and the table's own ends)
        for (int ax = 0; ax < 3; ++ax) {
            const int ks[] = {0, 1, lo_pad - 1, lo_pad, lo_pad + 1, (int)n[ax] - lo_pad - 1, (int)n[ax] - lo_pad,
                              (int)n[ax] - lo_pad + 1, (int)n[ax] - 1, (int)n[ax]};
            for (int k : ks) {
                const double face = o[ax] + (double)k / g.inv_h;
                const double cand[3] = {std::nextafter(face, -inf), face, std::nextafter(face, inf)};
                for (double v : cand)
                    for (int rep = 0; rep < 8; ++rep) {
                        double p[3];
                        for (int j = 0; j < 3; ++j) p[j] = o[j] + ((double)lo_pad + uni() * (double)(n[j] - 2 * lo_pad)) * h;
                        p[ax] = v;
                        same_as_parent(g, p[0], p[1], p[2], lo_pad);
                    }
            }
        }
    printf("%s: n %u %u %u inv_h %.17g K %d: %llu inside, %llu rejected\n", name, g.nx, g.ny, g.nz, g.inv_h, g.K,
           (unsigned long long)(n_in - in0), (unsigned long long)(n_out - out0));
    CHECK(n_in - in0 > 100000 && n_out - out0 > 100000);   // (both outcomes are exercised)
}

static Desc radius_desc(const RadiusGridGeom& geom) {   // radius_grid_desc (m3d_device.cpp)
    Desc g;
    g.K = geom.K;
    g.ox = geom.origin[0];
    g.oy = geom.origin[1];
    g.oz = geom.origin[2];
    g.inv_h = 1.0 / geom.h;
    g.nx = (uint32_t)geom.dims[0];
    g.ny = (uint32_t)geom.dims[1];
    g.nz = (uint32_t)geom.dims[2];
    return g;
}

// one query of [lo - edge, hi + edge]: a cell with lo_pad = K, and every x-row span of its block inside the table
static void query_fits(const Desc& g, const double q[3]) {
    int ix, iy, iz;
    const bool ok = grid_cell(g, q[0], q[1], q[2], g.K, &ix, &iy, &iz);
    CHECK(ok);
    if (!ok) return;
    const int64_t ncell = (int64_t)g.nx * g.ny * g.nz;
    for (int dz = -g.K; dz <= g.K; ++dz)
        for (int dy = -g.K; dy <= g.K; ++dy) {
            CHECK(iy + dy >= 0 && iy + dy < (int)g.ny && iz + dz >= 0 && iz + dz < (int)g.nz);
            const int64_t row = (int64_t)grid_cell_id(g, ix, iy + dy, iz + dz);
            CHECK(row == ((int64_t)(iz + dz) * g.ny + (iy + dy)) * g.nx + ix);
            CHECK(row - g.K >= 0 && row + g.K + 1 <= ncell);                      // the indices grid_row_span reads
            CHECK(ix - g.K >= 0 && ix + g.K < (int)g.nx);                         // ... and they stay in this x-row
        }
}

struct Row {
    double lo[3], hi[3], edge;
    int K0, K;
};

int main() {
    const Row rows[] = {
        {{0, 0, 0}, {1, 2, 3}, 0.5, 4, 4},                 // (the rows of test_grid_geom.cpp)
        {{0, 0, 0}, {1, 2, 3}, 0.5, 1, 1},
        {{0, 0, 0}, {1000, 1000, 1000}, 0.5, 4, 1},        // K halved twice, the cell doubled four times
        {{-1, -1, -1}, {-1, -1, -1}, 0.25, 1, 1},          // a single point
        {{0, 0, 0}, {100, 100, 100}, 0.5, 4, 2},           // K halved once: 410^3 cells
        // K0 no power of two (the registration's rule gives any of 1..16), after a forced halving
        {{0, 0, 0}, {100, 100, 100}, 0.5, 3, 1},           // 3 -> 1
        {{0, 0, 0}, {100, 100, 100}, 0.5, 5, 2},           // 5 -> 2
        {{0, 0, 0}, {80, 80, 80}, 0.5, 6, 3},              // 6 -> 3
        {{0, 0, 0}, {80, 80, 80}, 0.5, 7, 3},              // 7 -> 3
        {{0, 0, 0}, {80, 80, 80}, 0.5, 12, 3},             // 12 -> 6 -> 3
        {{0, 0, 0}, {100, 100, 100}, 0.5, 12, 1},          // 12 -> 6 -> 3 -> 1
    };
    for (const Row& r : rows) {
        const RadiusGridGeom geom = radius_grid_geom(r.lo, r.hi, r.edge, r.K0);
        CHECK(geom.K == r.K && std::isfinite(geom.h));
        const Desc g = radius_desc(geom);
        compare(g, "radius grid");
        // ---- the padding contract
        const double f[] = {0.0, 1.0, 0.5, 0x1p-53, 1.0 - 0x1p-53};   // the box's ends, its middle, next to the ends
        for (double fx : f)
            for (double fy : f)
                for (double fz : f) {
                    const double t[3] = {fx, fy, fz};
                    double p[3], q[3];
                    for (int k = 0; k < 3; ++k) {
                        p[k] = t[k] == 0.0 ? r.lo[k] : (t[k] == 1.0 ? r.hi[k] : r.lo[k] + t[k] * (r.hi[k] - r.lo[k]));
                        q[k] = t[k] == 0.0 ? r.lo[k] - r.edge
                                           : (t[k] == 1.0 ? r.hi[k] + r.edge
                                                          : (r.lo[k] - r.edge) + t[k] * ((r.hi[k] + r.edge) - (r.lo[k] - r.edge)));
                    }
                    int ix, iy, iz;
                    CHECK(grid_cell(g, p[0], p[1], p[2], 0, &ix, &iy, &iz));
                    query_fits(g, q);
                }
        for (int i = 0; i < 20000; ++i) {
            double p[3], q[3];
            for (int k = 0; k < 3; ++k) {
                p[k] = r.lo[k] + uni() * (r.hi[k] - r.lo[k]);
                q[k] = (r.lo[k] - r.edge) + uni() * ((r.hi[k] + r.edge) - (r.lo[k] - r.edge));
                if (p[k] > r.hi[k]) p[k] = r.hi[k];
                if (q[k] > r.hi[k] + r.edge) q[k] = r.hi[k] + r.edge;
            }
            int ix, iy, iz;
            CHECK(grid_cell(g, p[0], p[1], p[2], 0, &ix, &iy, &iz));
            query_fits(g, q);
            // ... and the block covers the edge: a query one edge from p along any diagonal has p's cell within K cells of its own
            int jx, jy, jz;
            for (int k = 0; k < 3; ++k) q[k] = p[k] + (((i >> k) & 1) ? r.edge : -r.edge);
            CHECK(grid_cell(g, q[0], q[1], q[2], g.K, &jx, &jy, &jz));
            CHECK(std::abs(jx - ix) <= g.K && std::abs(jy - iy) <= g.K && std::abs(jz - iz) <= g.K);
        }
    }
    {   // a Hilbert sort's descriptor (hilbert_sort_desc): 2^bits cells per axis from the box's corner, no pads
        Desc g;
        g.K = 1;
        g.ox = -0.1;
        g.oy = 0.2;
        g.oz = 3.0;
        g.inv_h = sort_grid_inv_h(0.3, 6);
        g.nx = g.ny = g.nz = 1u << 6;
        compare(g, "hilbert sort");
        int ix, iy, iz;   // the far face of the largest extent is inside the last cell (the 1e-9 of sort_grid_inv_h)
        CHECK(grid_cell(g, g.ox + 0.3, g.oy + 0.3, g.oz + 0.3, 0, &ix, &iy, &iz) && ix == 63 && iy == 63 && iz == 63);
    }
    {   // the row-major id and the x-row span, by hand: nx 26, ny 34, nz 42
        Desc g{};
        g.nx = 26;
        g.ny = 34;
        g.nz = 42;
        CHECK(grid_cell_id(g, 0, 0, 0) == 0u);
        CHECK(grid_cell_id(g, 1, 0, 0) == 1u);
        CHECK(grid_cell_id(g, 0, 1, 0) == 26u);
        CHECK(grid_cell_id(g, 0, 0, 1) == 884u);
        CHECK(grid_cell_id(g, 3, 5, 7) == 6321u);     // (7 * 34 + 5) * 26 + 3
        CHECK(grid_cell_id(g, 25, 33, 41) == 37127u);   // 26 * 34 * 42 - 1
        std::vector<uint32_t> cs(64);
        for (uint32_t i = 0; i < 64; ++i) cs[i] = 3u * i + (i & 1u);
        uint32_t b = 0, e = 0;
        grid_row_span(cs.data(), 10u, -1, 1, &b, &e);
        CHECK(b == cs[9] && e == cs[12]);
        grid_row_span(cs.data(), 10u, -4, 4, &b, &e);
        CHECK(b == cs[6] && e == cs[15]);
        grid_row_span(cs.data(), 20u, 2, 2, &b, &e);
        CHECK(b == cs[22] && e == cs[23]);
    }
    printf(bad ? "FAILED: %d checks\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
