// m3d_fps.hpp -- launchers of the farthest point sampling kernels (m3d_fps.hip), called by m3d_preprocessing.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace m3d {

// (a) one workgroup of 1024 threads holds the whole cloud in VGPRs and runs all S steps in one launch
constexpr uint32_t kFpsSingleThreads = 1024;
constexpr uint32_t kFpsSingleMaxPoints = 8 * kFpsSingleThreads;   // 8 points per thread at most (16 spill: 128 VGPRs + scratch)
// out[0 .. S-1] = the sampled indices.  aos: n x 3 doubles on the device, 1 <= S <= n <= kFpsSingleMaxPoints.
void launch_fps_single(const double* aos, uint32_t n, uint32_t S, uint32_t* out, hipStream_t st);

// (b) tile-pruned steps over Hilbert-sorted 512-point tiles, one launch per sample
struct FpsState {          // the device's running state of a call (one 64-byte block)
    double sel[3];         // the point selected last
    uint32_t farthest;     // ... and its original index
    uint32_t ticket;       // last-arriver ticket of the step in flight (zero between steps)
    unsigned long long tiles_updated;   // tiles the steps updated (pruning statistics)
    uint32_t pad[6];
};
constexpr int kFpsTileDoubles = 8;   // per tile: lo xyz, hi xyz, tmax, tidx (uint32 in the bits of the last double)
// per tile: the exact box of its points, dist = +inf for its points (0 for padding slots: orig = 0xFFFFFFFF), and the
// record (tmax, tidx) = (+inf, lowest original index) or (0, -) for a tile of padding only
void launch_fps_tiles_init(const double* sx, const double* sy, const double* sz, const uint32_t* orig, uint32_t n_tiles,
                           double* dist, double* tiles, hipStream_t st);
// grid of the step kernel for n_tiles tiles (wg_rec holds 2 doubles per workgroup of it)
uint32_t fps_step_grid(uint32_t n_tiles);
// one step: update with the selected point of `state`, select the next one (lowest original index among the largest
// distances; nf_idx: the lowest index of a point left out of the tiles for a non-finite coordinate -- a constant +inf
// candidate -- or 0xFFFFFFFF), write out[i] and the state's point.  prune = false: every tile is updated (the dense form).
void launch_fps_step(const double* aos, const double* sx, const double* sy, const double* sz, const uint32_t* orig,
                     uint32_t n_tiles, double* dist, double* tiles, double* wg_rec, FpsState* state, uint32_t nf_idx,
                     uint32_t* out, uint32_t i, bool prune, hipStream_t st);

}  // namespace m3d
