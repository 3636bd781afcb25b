// m3d_grid_geom.hpp -- the host arithmetic behind every cell-sorted grid (CellSort, m3d_driver.hpp): the dimensions of the
// radius grids (registration's target grid, boundary detection, ProximityExtractor) and the resolution of the Hilbert sorts
// (m3d_cloud_create, farthest point sampling).  Plain C++, no HIP: tests/cpp/test_grid_geom.cpp compiles it with g++ and pins
// it bit for bit.  Compile with -ffp-contract=off, as everything else here.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace m3d {

struct RadiusGridGeom {
    int K;               // cells per `edge` that fitted
    double h;            // cell edge (not finite: no cell edge holds the extent -- one cell per axis + pads)
    uint64_t dims[3];    // cells per axis, 2K + 1 pad cells per side included
    double origin[3];    // lo - (2K + 1) h
};

// Uniform grid over the box [lo, hi] for searches within `edge`: cell edge h = 1.001 edge / K with K = K0, K0 / 2, ... 1 while
// the dense cell table does not fit (<= 2^27 cells, < 1e9 per axis), h recomputed from the halved K (K0 need be no power of two:
// reg_grid_k0 below gives any of 1..16); if even K = 1 does not fit the cell is doubled (a coarser grid with K = 1 still covers
// the edge).  The invariant every search rests on: K h >= 1.001 edge at every rung, so the (2K + 1)^3 block of cells around a
// query's cell holds everything within `edge` of it.  For K0 a power of two the rungs are bit for bit those of doubling h at every
// step (tests/cpp/test_grid_geom.cpp holds both).  2K + 1 pad cells on every side: a query up to one edge (< K cells) outside the box
// still has its whole (2K + 1)^3 search block inside the table, and anything further out cannot have a neighbour.
// edge > 0 (a zero edge would never fit).  The order of the operations is part of the interface.
inline RadiusGridGeom radius_grid_geom(const double lo[3], const double hi[3], double edge, int K0) {
    RadiusGridGeom g;
    int K = K0;
    double h = edge * 1.001 / K;
    for (;;) {
        if (!std::isfinite(h)) {   // (an infinite cell holds any box: what the division below gives for a finite extent)
            for (int k = 0; k < 3; ++k) g.dims[k] = 1 + 2 * (uint64_t)(2 * K + 1);
            break;
        }
        bool fits = true;
        uint64_t cells = 1;
        for (int k = 0; k < 3; ++k) {
            const double ext = (hi[k] - lo[k]) / h;
            if (!(ext < 1e9)) {
                fits = false;
                break;
            }
            g.dims[k] = (uint64_t)ext + 1 + 2 * (uint64_t)(2 * K + 1);
            cells *= g.dims[k];
            if (cells > ((uint64_t)1 << 27)) fits = false;
        }
        if (fits) break;
        if (K > 1) {
            K /= 2;
            h = edge * 1.001 / K;   // (not h * 2: K0 / 2 rounds down for an odd K0, and K cells must still cover the edge)
        } else {
            h *= 2.0;
        }
    }
    g.K = K;
    g.h = h;
    for (int k = 0; k < 3; ++k) g.origin[k] = lo[k] - (2 * K + 1) * h;
    return g;
}

// K0 of the registration validation's grid: k_cfg (m3d_config.reg_cells_per_radius) is the figure for a 200 000-point target; a
// smaller one gets coarser cells in proportion to the cube root (about the same points per cell), a larger one keeps k_cfg.
// Any integer of 1 .. k_cfg may result, not only powers of two.
inline int reg_grid_k0(int k_cfg, uint64_t n_dst) {
    return std::max(1, std::min(k_cfg, (int)std::lround(k_cfg * std::cbrt((double)n_dst / 200000.0))));
}

// Hilbert sorts of a whole cloud: 2^bits cells per axis, about 8 points per cell, at most 2^8 per axis
inline uint32_t sort_grid_bits(uint64_t n_finite) {
    uint32_t bits = 1;
    while (bits < 8 && ((uint64_t)1 << (3 * bits)) * 8 < n_finite) ++bits;
    return bits;
}
// ... and their cells per unit length over the largest extent `ext` of the box (the 1e-9 keeps the far face inside the last cell;
// 0: a single point or an absurdly large cloud -- everything in cell 0)
inline double sort_grid_inv_h(double ext, uint32_t bits) {
    return ext > 0.0 ? (double)(1u << bits) / (ext * (1.0 + 1e-9)) : 0.0;
}

}  // namespace m3d
