// m3d_proximity.hpp -- launchers of ProximityExtractor's kernels (m3d_proximity.hip), called by m3d_proximity.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "m3d_proximity_fp.hpp"
#include "m3d_reg_kernels.hpp"

namespace m3d {

// parent[i] = i, size[i] = 0 for i < n
void launch_prox_init(uint32_t* parent, uint32_t* size, uint32_t n, hipStream_t st);
// sorted copies of the normals next to the grid's qx / qy / qz: sn[t] = normals[cell_orig[t]] for t < n_sorted[0]
void launch_prox_gather_normals(const CloudView& c, const uint32_t* cell_orig, uint32_t n, const uint32_t* n_sorted,
                                double* snx, double* sny, double* snz, hipStream_t st);
// the radius graph over the grid (cell >= radius, K = 1): every unordered pair within the radius that the evaluator
// accepts is united in parent[] (original indices; a root is the smallest index of its tree)
void launch_prox_union_grid(const GridDesc& g, const uint32_t* cell_start, const double* qx, const double* qy,
                            const double* qz, const uint32_t* cell_orig, const double* snx, const double* sny,
                            const double* snz, uint32_t n, const uint32_t* n_sorted, const ProxCut& cut, uint32_t* parent,
                            hipStream_t st);
// the caller's lists (CSR, entry 0 of every list skipped): edge i -> idx[k] for k in [off[i] + 1, off[i + 1]), dist =
// norm3(p_i - p_j), every index already checked to lie in [0, n)
void launch_prox_union_lists(const CloudView& c, const uint64_t* off, const uint32_t* idx, uint32_t n, const ProxCut& cut,
                             uint32_t* parent, hipStream_t st);
// root[i] = the root of i (the union launches have ended: plain loads), size[root] += 1
void launch_prox_flatten(const uint32_t* parent, uint32_t* root, uint32_t* size, uint32_t n, hipStream_t st);
// radius neighbour lists (self excluded): count[i] = |N(i)|; then with off (exclusive prefix of count, n + 1 entries) the
// lists themselves, each sorted by (d2, index)
void launch_prox_nb_count(const GridDesc& g, const uint32_t* cell_start, const double* qx, const double* qy, const double* qz,
                          const uint32_t* cell_orig, uint32_t n, const uint32_t* n_sorted, uint32_t* count, hipStream_t st);
void launch_prox_nb_fill(const GridDesc& g, const uint32_t* cell_start, const double* qx, const double* qy, const double* qz,
                         const uint32_t* cell_orig, uint32_t n, const uint32_t* n_sorted, const uint64_t* off,
                         uint32_t* nb_idx, double* nb_d2, hipStream_t st);

}  // namespace m3d
