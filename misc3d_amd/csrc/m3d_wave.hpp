// m3d_wave.hpp -- reductions and the prefix sum over the 64 lanes of a wave (device only).
//
// wave_reduce is an xor butterfly from WIDTH / 2 down to 1: lane l combines with lane l ^ 32, then l ^ 16, ... l ^ 1, and every
// lane of an aligned group of WIDTH ends with the same value.  THE ORDER IS PART OF THE INTERFACE: several callers sum fp64
// numbers (reg_validate_k's distance sums, tile_frames_k's moments) and their results are compared bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace m3d {

// (the unsigned types travel through the shuffles' signed overloads)
__device__ __forceinline__ uint32_t lane_xor(uint32_t v, int off) { return (uint32_t)__shfl_xor((int)v, off, 64); }
__device__ __forceinline__ unsigned long long lane_xor(unsigned long long v, int off) {
    return (unsigned long long)__shfl_xor((long long)v, off, 64);
}
__device__ __forceinline__ float lane_xor(float v, int off) { return __shfl_xor(v, off, 64); }
__device__ __forceinline__ double lane_xor(double v, int off) { return __shfl_xor(v, off, 64); }

template <int WIDTH = 64, class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
    static_assert(WIDTH >= 2 && WIDTH <= 64 && (WIDTH & (WIDTH - 1)) == 0, "a power of two of lanes");
    for (int off = WIDTH / 2; off > 0; off >>= 1) v = op(v, lane_xor(v, off));
    return v;
}

// integers: min / max; float: fminf / fmaxf; double: fmin / fmax (a NaN operand is dropped, as at every caller before)
__device__ __forceinline__ uint32_t lane_min(uint32_t a, uint32_t b) { return min(a, b); }
__device__ __forceinline__ unsigned long long lane_min(unsigned long long a, unsigned long long b) { return min(a, b); }
__device__ __forceinline__ float lane_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double lane_min(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ uint32_t lane_max(uint32_t a, uint32_t b) { return max(a, b); }
__device__ __forceinline__ unsigned long long lane_max(unsigned long long a, unsigned long long b) { return max(a, b); }
__device__ __forceinline__ float lane_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double lane_max(double a, double b) { return fmax(a, b); }

// T: uint32_t, unsigned long long, float, double
template <int WIDTH = 64, class T>
__device__ __forceinline__ T wave_sum(T v) {
    return wave_reduce<WIDTH>(v, [](T a, T b) { return a + b; });
}
template <int WIDTH = 64, class T>
__device__ __forceinline__ T wave_min(T v) {
    return wave_reduce<WIDTH>(v, [](T a, T b) { return lane_min(a, b); });
}
template <int WIDTH = 64, class T>
__device__ __forceinline__ T wave_max(T v) {
    return wave_reduce<WIDTH>(v, [](T a, T b) { return lane_max(a, b); });
}

// inclusive prefix sum over the wave's lanes; lane = the caller's lane index (0 .. 63)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

}  // namespace m3d
