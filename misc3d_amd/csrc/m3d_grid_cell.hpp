// m3d_grid_cell.hpp -- the cell of a point in a cell-sorted grid, its row-major id and the span of an x-row: ONE definition
// for the kernel that assigns the points to cells (grid_count_k) and for every search that looks them up (registration, its
// candidate cache, boundary detection, ProximityExtractor) -- they must agree bit for bit, or a query looks in the wrong cell.
// Host and device, plain C++: tests/cpp/test_grid_cell.cpp compiles it with g++ (-ffp-contract=off).
// G: anything with ox, oy, oz, inv_h and nx, ny, nz (GridDesc, m3d_reg_kernels.hpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef M3D_HD
#define M3D_HD __host__ __device__ __forceinline__
#endif
#else
#ifndef M3D_HD
#define M3D_HD inline
#endif
#endif

namespace m3d {

// The cell of (x, y, z) and the position inside it as a fraction of the cell edge; false, and nothing written, outside
// [lo_pad, n - lo_pad) on some axis.  The scaled coordinate is (x - o) * inv_h, TWO roundings and no fused operation: relative
// error < 3 * 2^-53 of a value below 2^27, below 5e-8 cell edges -- the 1e-6 slack of axis_gap (m3d_reg_kernels.hip) rests on it.
// lo_pad = 0 admits every cell of the table (the points of the cloud); a query passes lo_pad = K: the table carries 2K + 1
// pad cells per side (m3d_grid_geom.hpp), so every query within K cells of the bounding box is admitted and its (2K + 1)^3
// block stays inside the table.  NaN fails every comparison.
template <class G>
M3D_HD bool grid_cell_frac(const G& g, double x, double y, double z, int lo_pad, int* ix, int* iy, int* iz, double* frx,
                           double* fry, double* frz) {
    const double fx = (x - g.ox) * g.inv_h, fy = (y - g.oy) * g.inv_h, fz = (z - g.oz) * g.inv_h;
    if (!(fx >= (double)lo_pad && fx < (double)(g.nx - lo_pad) && fy >= (double)lo_pad &&
          fy < (double)(g.ny - lo_pad) && fz >= (double)lo_pad && fz < (double)(g.nz - lo_pad)))
        return false;
    *ix = (int)fx;
    *iy = (int)fy;
    *iz = (int)fz;
    *frx = fx - (double)*ix;   // (what (int) dropped; exact: both share their leading bits)
    *fry = fy - (double)*iy;
    *frz = fz - (double)*iz;
    return true;
}
template <class G>
M3D_HD bool grid_cell(const G& g, double x, double y, double z, int lo_pad, int* ix, int* iy, int* iz) {
    double frx, fry, frz;
    return grid_cell_frac(g, x, y, z, lo_pad, ix, iy, iz, &frx, &fry, &frz);
}

// row-major id of cell (ix, iy, iz): x runs fastest
template <class G>
M3D_HD uint32_t grid_cell_id(const G& g, int ix, int iy, int iz) {
    return ((uint32_t)iz * g.ny + (uint32_t)iy) * g.nx + (uint32_t)ix;
}

// [*b, *e): the slots of cells row + lo .. row + hi of one x-row (cell_start: the exclusive scan of the cell sizes).
// lo may be negative: row + lo is uint32_t arithmetic, exact modulo 2^32 because the cell it names exists (row + lo >= 0).
M3D_HD void grid_row_span(const uint32_t* cell_start, uint32_t row, int lo, int hi, uint32_t* b, uint32_t* e) {
    *b = cell_start[row + lo];
    *e = cell_start[row + hi + 1];
}

}  // namespace m3d
