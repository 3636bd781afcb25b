// m3d_voxel.hpp -- launchers of the voxel down-sampling kernels (m3d_voxel.hip), called by m3d_voxel.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "m3d_radix_sort.hpp"   // the exclusive scan and the stable sort (their kernels are in m3d_voxel.hip)

namespace m3d {

constexpr uint32_t kVoxelNone = 0xFFFFFFFFu;
constexpr uint32_t kVoxelBoundsBlocks = 1024;   // partial records of the bounds reduction

struct VoxelBounds {   // what the bounds reduction leaves on the device (one 64-byte block)
    double lo[3], hi[3];       // coordinate-wise min / max over the points with three finite coordinates
    uint32_t first_nonfinite;  // lowest index of a point with a non-finite coordinate, kVoxelNone if there is none
    uint32_t pad[3];
};

struct VoxelGrid {   // a level's grid, computed on the host from the bounds (m3d_voxel.cpp)
    double vmin[3];
    double voxel_size;
    uint32_t bits[3];   // packed keys: bit widths of the three voxel indices (their sum <= 63); unused for wide keys
};

// partial: kVoxelBoundsBlocks records of scratch
void launch_voxel_bounds(const double* xyz, uint32_t n, VoxelBounds* partial, VoxelBounds* out, hipStream_t st);

// keys of the points: packed into key64[i] (wide == false), or the three indices in key96[3 i ..] (wide == true)
void launch_voxel_keys(const double* xyz, uint32_t n, const VoxelGrid& g, bool wide, unsigned long long* key64,
                       uint32_t* key96, hipStream_t st);
// One hash table of table_size (a power of two >= 2 n) slots, all bytes 0xFF on entry: table64 holds packed keys, table32
// (wide keys) the index of a member whose key96 stands for the slot.  slot_of[i] = the slot of point i's voxel,
// first[slot] = the lowest member index (first: table_size words, 0xFF on entry).
void launch_voxel_insert(uint32_t n, bool wide, const unsigned long long* key64, const uint32_t* key96,
                         unsigned long long* table64, uint32_t* table32, uint32_t table_size, uint32_t* first,
                         uint32_t* slot_of, hipStream_t st);
// is_first[i] = 1 when point i is the lowest member of its voxel, else 0
void launch_voxel_flags(uint32_t n, const uint32_t* slot_of, const uint32_t* first, uint32_t* is_first, hipStream_t st);
// rank = the exclusive scan of is_first: vid[i] = rank[first[slot_of[i]]] (the voxel's output row), first_index[vid] for
// the first members
void launch_voxel_ids(uint32_t n, const uint32_t* slot_of, const uint32_t* first, const uint32_t* rank, uint32_t* vid,
                      uint32_t* first_index, hipStream_t st);

// sorted_keys ascending: offsets[j] = the first position of voxel j, offsets[m] = n
void launch_voxel_offsets(const uint32_t* sorted_keys, uint32_t n, uint32_t m, uint32_t* offsets, hipStream_t st);
// per voxel j, its members order[offsets[j] .. offsets[j + 1]) (vals_sorted == nullptr: the identity) added one by one in
// that order, then divided by the count.  normals / colors and their outputs may be null.
void launch_voxel_means(const double* xyz, const double* normals, const double* colors, const uint32_t* order,
                        const uint32_t* offsets, uint32_t m, double* out_xyz, double* out_normals, double* out_colors,
                        hipStream_t st);

}  // namespace m3d
