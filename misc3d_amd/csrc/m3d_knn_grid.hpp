// m3d_knn_grid.hpp -- the dim-3 density grid of the k-NN grid path as the host driver holds it (built by m3d_knn.cpp),
// shared by KNearestSearch (m3d_knn.cpp) and the normals / FPFH driver (m3d_fpfh.cpp).  The device view and the kernel
// launchers are in m3d_knn.hpp.
#pragma once
#include "m3d_driver_internal.hpp"
#include "m3d_knn.hpp"

namespace m3d {

constexpr int kKnnGridClasses = 4;   // lists of <= 16, 32, 64, 128 pairs
int knn_grid_class(int kk);

struct KnnGrid {
    bool built = false, usable = false;
    KnnGridDesc g{};
    DevBuf cell_start, sx, sy, sz, sidx, slabs, out_rows;
    KnnGridView view() const;   // (data is left null: the caller points it at its n x 3 rows)
    void release();
};

// The grid of class cls over the finite rows of `rows` (n x 3 on the host), uploaded on the caller's lane and complete
// when the call returns.  G.usable is false when there is no finite row or the extent overflows.
int knn_build_grid(DeviceCtx* ctx, const double* rows, size_t n, int cls, KnnGrid& G);

}  // namespace m3d
