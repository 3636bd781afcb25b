// m3d_fpfh.hpp -- launchers of the normals / FPFH kernels (m3d_fpfh.hip), called by m3d_fpfh.cpp.
//
// Queries are the FINITE points in the order of the k-NN grid (cell-major: neighbours in space are neighbours in memory):
// query t is point sidx[t].  Its neighbour list is l_idx / l_d2[t kk + j], j < kk, ascending by (d2, index), as
// launch_knn_grid writes it; cnt[t] = how many leading entries are neighbours (finite d2, and d2 < r2 for Hybrid).
// Everything else -- xyz, normals, SPFH rows, the output -- is indexed by the point's own index.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace m3d {

// One SPFH row as the device keeps it: every increment of a row is the same incr = 100 / (m - 1), so the row is its
// pair counts (<= 127 each) and that one double: 48 bytes to gather where 33 doubles would be 264.
struct alignas(16) SpfhRow {
    double incr;
    uint8_t count[40];   // 33 used
};

// q3[t] = (sx[t], sy[t], sz[t]): the grid's sorted rows as launch_knn_grid's query array
void launch_fpfh_queries(const double* sx, const double* sy, const double* sz, uint32_t nq, double* q3, hipStream_t st);
// cnt[t] (above); *pairs += their sum
void launch_fpfh_count(const double* l_d2, uint32_t nq, int kk, int hybrid, double r2, uint32_t* cnt,
                       unsigned long long* pairs, hipStream_t st);
// normals[sidx[t]] from the covariance of the list (m < 3: (0, 0, 1)), oriented towards cam when orient != 0
void launch_fpfh_normals(const double* xyz, const uint32_t* sidx, const uint32_t* l_idx, const uint32_t* cnt, uint32_t nq,
                         int kk, int orient, const double* cam3 /* host */, double* normals, hipStream_t st);
// OrientNormalsTowardsCameraLocation over all n points, in place
void launch_fpfh_orient(const double* xyz, uint32_t n, const double* cam3 /* host */, double* normals, hipStream_t st);
// tie_list[0 .. *tie_count) (capacity nq, *tie_count zeroed by the caller): the queries t with a pair whose swap
// decision is a near tie of the two acos values (m3d_fpfh_fp.hpp kFpfhTieBand); their rows are redone by the host
void launch_fpfh_spfh(const double* xyz, const double* normals, const uint32_t* sidx, const uint32_t* l_idx,
                      const uint32_t* cnt, uint32_t nq, int kk, SpfhRow* spfh, uint32_t* tie_list, uint32_t* tie_count,
                      hipStream_t st);
// packed[e (2 + kk) ...] = (point index, m, the kk list entries) of query tie_list[e], e < n_ties
void launch_fpfh_tie_gather(const uint32_t* tie_list, uint32_t n_ties, const uint32_t* sidx, const uint32_t* l_idx,
                            const uint32_t* cnt, int kk, uint32_t* packed, hipStream_t st);
// spfh[points[e]] = rows[e], e < n_ties
void launch_fpfh_tie_scatter(const uint32_t* points, const SpfhRow* rows, uint32_t n_ties, SpfhRow* spfh, hipStream_t st);
// out[sidx[t] 33 + j]; rows of points that are no query are not written (the caller zeroes out)
void launch_fpfh_fpfh(const SpfhRow* spfh, const uint32_t* sidx, const uint32_t* l_idx, const double* l_d2,
                      const uint32_t* cnt, uint32_t nq, int kk, double* out, hipStream_t st);

}  // namespace m3d
