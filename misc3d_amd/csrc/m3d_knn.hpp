// m3d_knn.hpp -- launchers of KNearestSearch's kernels (m3d_knn.hip), called by m3d_knn.cpp.
//
// Keys: a row r of query q is ranked by (key(d2), r), both ascending, where d2 is the serial fp64 sum of
// include/misc3d_amd.h and key(d2) = the bits of d2 (d2 is +0, positive or +inf: its bits order as the values do) or
// kKnnNanKey for a NaN d2.  Every (key, index) pair is distinct, so "the kout smallest pairs" is one set in one order.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace m3d {

constexpr uint64_t kKnnNanKey = 0x7FF8000000000000ull;   // the canonical quiet NaN: above +inf's bits
constexpr int kKnnPageMax = 128;                          // longest per-query list of the tile and grid kernels
constexpr int kKnnTileRows = 32;                          // rows per LDS tile
constexpr int kKnnTileDims = 16;                          // dimensions per LDS tile
constexpr int kKnnMaxSplits = 256;                        // database splits per query (merge: four lists per lane)

// The dim-3 density grid: the finite rows counting-sorted by cell (sx / sy / sz / sidx, cell_start), per axis the
// prefix maximum / suffix minimum of the coordinate over the slabs of cells (pmax[a][c] = max p_a over the sorted rows
// whose cell index on axis a is <= c; smin[a][c] = min over cell index >= c; -inf / +inf where there are none), and the
// rows with a non-finite coordinate (every query scans them).
struct KnnGridDesc {
    double ox, oy, oz, inv_h;
    int32_t nx, ny, nz;
    uint32_t n_out;   // rows with a non-finite coordinate (out_rows)
};
struct KnnGridView {
    KnnGridDesc g;
    const uint32_t* cell_start;   // nx ny nz + 1
    const double *sx, *sy, *sz;
    const uint32_t* sidx;
    const double* pmax[3];
    const double* smin[3];
    const uint32_t* out_rows;
    const double* data;   // n x 3, row-major (the non-finite rows are read from here)
};

// Brute force over the rows of each split: part_key / part_idx[(q S + s) kk + j], j < kk, the kk smallest (key, index)
// of split s (rows [s rows_per_split, (s + 1) rows_per_split) & [0, n)) for query q (column q of qT, dim x mc), sentinel
// (~0, ~0) where the split has fewer.  floor (2 words per query: key, index) != null: only pairs above the floor count.
void launch_knn_tile(const double* data, uint32_t n, int dim, const double* qT, uint32_t mc, int kk, int splits,
                     uint32_t rows_per_split, const uint64_t* floor, uint64_t* part_key, uint32_t* part_idx, hipStream_t st);
// The S lists of each query merged: out_d2 / out_idx[q kk + o], o < kk; floor (may be null) = the last pair per query.
void launch_knn_merge(const uint64_t* part_key, const uint32_t* part_idx, uint32_t mc, int kk, int splits, uint64_t* floor,
                      double* out_d2, uint32_t* out_idx, hipStream_t st);
// dim 3, finite queries (q3: mc x 3): shells of grid cells until the kk-th pair is final (m3d_knn.hip), then the
// non-finite rows.  Output as launch_knn_merge's; pairs_seen += the rows whose distance was evaluated.
void launch_knn_grid(const KnnGridView& v, const double* q3, uint32_t mc, int kk, double* out_d2, uint32_t* out_idx,
                     unsigned long long* pairs_seen, hipStream_t st);

}  // namespace m3d
