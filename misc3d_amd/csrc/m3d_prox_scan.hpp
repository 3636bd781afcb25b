// m3d_prox_scan.hpp -- the scan of a point's 3x3x3 block in a radius grid whose cell edge covers the radius (K = 1), ONE
// definition for the kernels that walk the radius graph: ProximityExtractor (m3d_proximity.hip) and the normal orientation of
// the PPF model preprocessing (m3d_orient.hip).  Device only.
#pragma once
#include <hip/hip_runtime.h>

#include "m3d_grid_cell.hpp"
#include "m3d_proximity_fp.hpp"
#include "m3d_reg_kernels.hpp"

#pragma clang fp contract(off)

namespace m3d {

// visit(u, d2) for every grid slot u of the 3x3x3 block around sorted point t whose d2 is within the radius (t included)
template <class F>
__device__ __forceinline__ void prox_scan_block(const GridDesc& g, const uint32_t* __restrict__ cell_start,
                                                const double* __restrict__ qx, const double* __restrict__ qy,
                                                const double* __restrict__ qz, uint32_t t, F visit) {
    const double px = qx[t], py = qy[t], pz = qz[t];
    int ix, iy, iz;
    if (!grid_cell(g, px, py, pz, 1, &ix, &iy, &iz)) return;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy) {
            uint32_t b, e;
            grid_row_span(cell_start, grid_cell_id(g, ix, iy + dy, iz + dz), -1, 1, &b, &e);
            for (uint32_t u = b; u < e; ++u) {
                const double d2 = prox_d2(px - qx[u], py - qy[u], pz - qz[u]);
                if (prox_in_radius(d2, g.r2)) visit(u, d2);
            }
        }
}

}  // namespace m3d
