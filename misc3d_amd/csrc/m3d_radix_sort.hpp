// m3d_radix_sort.hpp -- the exclusive scan of uint32 and the stable LSD radix sort (8 bits a pass) of (key, value) pairs that
// voxel down-sampling (m3d_voxel.cpp: point indices by output row) and ray casting (m3d_raycast.cpp: triangles by Morton
// code) share.  The kernels are in m3d_voxel.hip.  Stable: equal keys keep the order of their values, so a sort whose
// values start as 0 .. n - 1 orders by (key, index).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace m3d {

constexpr uint32_t kVoxelScanTile = 2048;       // elements one workgroup of the scan handles
constexpr uint32_t kVoxelSortRadix = 256;       // 8 bits per pass of the stable sort
constexpr uint32_t kVoxelSortMaxBlocks = 8192;

// elements of the scratch scan_exclusive needs for n elements
size_t voxel_scan_scratch(size_t n);
// out[i] = in[0] + ... + in[i - 1], *total_dev = the sum of all (in == out allowed); uint32 arithmetic
void launch_scan_exclusive(const uint32_t* in, uint32_t* out, size_t n, uint32_t* scratch, uint32_t* total_dev, hipStream_t st);

// the stable sort's geometry for n elements: elements per workgroup (a multiple of 64) and workgroups
void voxel_sort_shape(uint32_t n, uint32_t* tile, uint32_t* blocks);
// one pass over the digit (key >> shift) & 255: counts[digit * blocks + block]
void launch_voxel_sort_count(const uint32_t* keys, uint32_t n, uint32_t shift, uint32_t* counts, hipStream_t st);
// ... counts scanned exclusively: a stable scatter of (keys, vals) (vals_in == nullptr: vals = 0 .. n - 1)
void launch_voxel_sort_scatter(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t n, uint32_t shift,
                               const uint32_t* counts, uint32_t* keys_out, uint32_t* vals_out, hipStream_t st);


// The whole sort: `passes` passes over the low 8 * passes bits of keys (vals == nullptr: the values start as 0 .. n - 1).
// k0 / v0 and k1 / v1: n words each, the passes' outputs in turn (k1 / v1 unused for one pass); counts: kVoxelSortRadix x
// the blocks of voxel_sort_shape(n); scan: voxel_scan_scratch(that many) words; total: one word.  The sorted pairs are
// in *keys_out / *vals_out (the inputs themselves for zero passes: then *vals_out may be nullptr = the identity).
inline void launch_radix_sort_pairs(const uint32_t* keys, const uint32_t* vals, uint32_t n, uint32_t passes, uint32_t* k0,
                                    uint32_t* v0, uint32_t* k1, uint32_t* v1, uint32_t* counts, uint32_t* scan, uint32_t* total,
                                    const uint32_t** keys_out, const uint32_t** vals_out, hipStream_t st) {
    uint32_t tile = 0, blocks = 0;
    voxel_sort_shape(n, &tile, &blocks);
    const size_t n_counts = (size_t)kVoxelSortRadix * blocks;
    for (uint32_t p = 0; p < passes; ++p) {
        uint32_t* ko = p & 1 ? k1 : k0;
        uint32_t* vo = p & 1 ? v1 : v0;
        launch_voxel_sort_count(keys, n, 8 * p, counts, st);
        launch_scan_exclusive(counts, counts, n_counts, scan, total, st);
        launch_voxel_sort_scatter(keys, vals, n, 8 * p, counts, ko, vo, st);
        keys = ko;
        vals = vo;
    }
    *keys_out = keys;
    *vals_out = vals;
}

}  // namespace m3d
