// m3d_voxel.hip -- voxel down-sampling (open3d::geometry::PointCloud::VoxelDownSample, the first call of every example
// of the reference and of MultiScaleICP, src/pipeline.cpp:937-938) on gfx950.
//
// The contract ([RECALL] Open3D 0.15.1 PointCloud::VoxelDownSample / AccumulatedPoint; DESIGN.md "Voxel down-sampling"):
//   vmin = min_bound - voxel_size * 0.5;  voxel of p = int(floor((p - vmin) / voxel_size)) per coordinate -- one
//   subtraction, one IEEE DIVISION, floor; per voxel the members' coordinates (normals, colours) are added one by one
//   in ascending point index from +0.0 (a normal with a NaN component is left out) and divided by double(count).
// The output order is ours: voxels in ascending order of their lowest member index.
//
// Nothing here depends on M3D_FP_ORDER: a sum never has more than two operands.
//
// How the members of a voxel get added in index order without fp64 atomics or trees:
//   1. voxel_keys_k      the three indices of every point (packed into 64 bits when their widths allow, else 3 x 32)
//   2. voxel_insert_k    an open-addressing hash table over the keys; atomicMin leaves every slot's lowest member index
//   3. voxel_flags_k + scan + voxel_ids_k   the voxels ranked by that index: vid[i] = output row of point i
//   4. voxel_sort_*      a stable LSD radix sort of the point indices by vid (8 bits a pass, ceil(log2 m / 8) passes):
//                        stable, so inside a voxel the indices stay ascending
//   5. voxel_means_k     one wave per voxel: 64 members at a time are gathered into LDS by all lanes, then lane c adds
//                        component c serially (9 independent chains at most: xyz, normal, colour)
// Integers (keys, counts, ranks) are computed in any order; every fp64 sum is one lane's serial chain.
#include "m3d_voxel.hpp"

namespace m3d {

namespace {

constexpr unsigned long long kEmpty64 = ~0ull;

__device__ __forceinline__ uint32_t load_relaxed(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long load_relaxed(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long h) {   // (murmur3's finaliser)
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}

// ---- bounds ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void bounds_merge(VoxelBounds& a, const VoxelBounds& b) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a.lo[c] = b.lo[c] < a.lo[c] ? b.lo[c] : a.lo[c];
        a.hi[c] = b.hi[c] > a.hi[c] ? b.hi[c] : a.hi[c];
    }
    a.first_nonfinite = b.first_nonfinite < a.first_nonfinite ? b.first_nonfinite : a.first_nonfinite;
}

__device__ __forceinline__ VoxelBounds bounds_empty() {
    VoxelBounds r;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        r.lo[c] = __builtin_inf();
        r.hi[c] = -__builtin_inf();
    }
    r.first_nonfinite = kVoxelNone;
    r.pad[0] = r.pad[1] = r.pad[2] = 0;
    return r;
}

// the workgroup's 256 records folded into thread 0's
__device__ __forceinline__ void bounds_block_fold(VoxelBounds& r, VoxelBounds* s) {
    const uint32_t tid = threadIdx.x;
    s[tid] = r;
    __syncthreads();
    for (uint32_t w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            bounds_merge(r, s[tid + w]);
            s[tid] = r;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void voxel_bounds_k(const double* __restrict__ xyz, uint32_t n, VoxelBounds* __restrict__ partial) {
    __shared__ VoxelBounds s[256];
    VoxelBounds r = bounds_empty();
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        if (isfinite(x) && isfinite(y) && isfinite(z)) {
            r.lo[0] = x < r.lo[0] ? x : r.lo[0];
            r.lo[1] = y < r.lo[1] ? y : r.lo[1];
            r.lo[2] = z < r.lo[2] ? z : r.lo[2];
            r.hi[0] = x > r.hi[0] ? x : r.hi[0];
            r.hi[1] = y > r.hi[1] ? y : r.hi[1];
            r.hi[2] = z > r.hi[2] ? z : r.hi[2];
        } else if ((uint32_t)i < r.first_nonfinite) {
            r.first_nonfinite = (uint32_t)i;
        }
    }
    bounds_block_fold(r, s);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

__global__ __launch_bounds__(256) void voxel_bounds_final_k(const VoxelBounds* __restrict__ partial, uint32_t n_partial,
                                                            VoxelBounds* __restrict__ out) {
    __shared__ VoxelBounds s[256];
    VoxelBounds r = bounds_empty();
    for (uint32_t i = threadIdx.x; i < n_partial; i += 256) bounds_merge(r, partial[i]);
    bounds_block_fold(r, s);
    if (threadIdx.x == 0) *out = r;
}

// ---- keys and the hash table --------------------------------------------------------------------------------------------
template <bool WIDE>
__global__ __launch_bounds__(256) void voxel_keys_k(const double* __restrict__ xyz, uint32_t n, VoxelGrid g,
                                                    unsigned long long* __restrict__ key64, uint32_t* __restrict__ key96) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t k[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double d = xyz[3 * i + c] - g.vmin[c];   // one subtraction,
        const double q = d / g.voxel_size;             // one IEEE division (a reciprocal moves points on voxel faces),
        k[c] = (uint32_t)(int)floor(q);                // floor, int: in [0, INT_MAX] by the host's checks
    }
    if (WIDE) {
        key96[3 * i] = k[0];
        key96[3 * i + 1] = k[1];
        key96[3 * i + 2] = k[2];
    } else {
        key64[i] = (unsigned long long)k[0] | ((unsigned long long)k[1] << g.bits[0]) |
                   ((unsigned long long)k[2] << (g.bits[0] + g.bits[1]));
    }
}

template <bool WIDE>
__global__ __launch_bounds__(256) void voxel_insert_k(uint32_t n, const unsigned long long* __restrict__ key64,
                                                      const uint32_t* __restrict__ key96, unsigned long long* table64,
                                                      uint32_t* table32, uint32_t mask, uint32_t* first,
                                                      uint32_t* __restrict__ slot_of) {
    const size_t gi = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= n) return;
    const uint32_t i = (uint32_t)gi;
    unsigned long long key = 0;
    uint32_t kx = 0, ky = 0, kz = 0;
    uint32_t slot;
    if (WIDE) {
        kx = key96[3 * gi];
        ky = key96[3 * gi + 1];
        kz = key96[3 * gi + 2];
        slot = (uint32_t)mix64(mix64(((unsigned long long)kx << 32) | ky) + kz) & mask;
    } else {
        key = key64[gi];
        slot = (uint32_t)mix64(key) & mask;
    }
    // linear probing; the table is at most half full, an entry never changes once it is set
    for (;;) {
        if (WIDE) {
            uint32_t cur = load_relaxed(&table32[slot]);
            if (cur == kVoxelNone) {
                const uint32_t old = atomicCAS(&table32[slot], kVoxelNone, i);
                cur = old == kVoxelNone ? i : old;
            }
            if (cur == i) break;
            // (key96 was written by the launch before this one)
            if (key96[3 * (size_t)cur] == kx && key96[3 * (size_t)cur + 1] == ky && key96[3 * (size_t)cur + 2] == kz) break;
        } else {
            unsigned long long cur = load_relaxed(&table64[slot]);
            if (cur == kEmpty64) {
                const unsigned long long old = atomicCAS(&table64[slot], kEmpty64, key);
                cur = old == kEmpty64 ? key : old;
            }
            if (cur == key) break;
        }
        slot = (slot + 1) & mask;
    }
    // the lowest member index; a stale read is an older, larger value and only costs the atomic
    if (load_relaxed(&first[slot]) > i) atomicMin(&first[slot], i);
    slot_of[gi] = slot;
}

__global__ __launch_bounds__(256) void voxel_flags_k(uint32_t n, const uint32_t* __restrict__ slot_of,
                                                     const uint32_t* __restrict__ first, uint32_t* __restrict__ is_first) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    is_first[i] = first[slot_of[i]] == (uint32_t)i ? 1u : 0u;
}

__global__ __launch_bounds__(256) void voxel_ids_k(uint32_t n, const uint32_t* __restrict__ slot_of,
                                                   const uint32_t* __restrict__ first, const uint32_t* __restrict__ rank,
                                                   uint32_t* __restrict__ vid, uint32_t* __restrict__ first_index) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = first[slot_of[i]];
    const uint32_t v = rank[f];
    vid[i] = v;
    if (f == (uint32_t)i) first_index[v] = f;
}

// ---- exclusive scan of uint32 -------------------------------------------------------------------------------------------
constexpr uint32_t kScanPerThread = kVoxelScanTile / 256;

// exclusive scan of the 256 threads' values through LDS; returns the thread's prefix, *total = the workgroup's sum
__device__ __forceinline__ uint32_t block_scan_256(uint32_t v, uint32_t* s, uint32_t* total) {
    const uint32_t tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {
        const uint32_t add = tid >= off ? s[tid - off] : 0u;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    const uint32_t incl = s[tid];
    *total = s[255];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(256) void scan_reduce_k(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ sums) {
    __shared__ uint32_t s[256];
    const size_t base = (size_t)blockIdx.x * kVoxelScanTile + (size_t)threadIdx.x * kScanPerThread;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanPerThread; ++k)
        if (base + k < n) v += in[base + k];
    uint32_t total;
    block_scan_256(v, s, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[0 .. nb) scanned exclusively in place, sums[nb] = *total_dev = the sum of all
__global__ __launch_bounds__(256) void scan_sums_k(uint32_t* __restrict__ sums, size_t nb, uint32_t* __restrict__ total_dev) {
    __shared__ uint32_t s[256];
    uint32_t carry = 0;
    for (size_t base = 0; base < nb; base += 256) {
        const size_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? sums[i] : 0u;
        uint32_t total;
        const uint32_t pre = block_scan_256(v, s, &total);
        if (i < nb) sums[i] = carry + pre;
        carry += total;
    }
    if (threadIdx.x == 0) {
        sums[nb] = carry;
        *total_dev = carry;
    }
}

__global__ __launch_bounds__(256) void scan_apply_k(const uint32_t* in, uint32_t* out, size_t n, const uint32_t* __restrict__ sums) {
    __shared__ uint32_t s[256];
    const size_t base = (size_t)blockIdx.x * kVoxelScanTile + (size_t)threadIdx.x * kScanPerThread;
    uint32_t v[kScanPerThread];
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanPerThread; ++k) {
        v[k] = base + k < n ? in[base + k] : 0u;
        sum += v[k];
    }
    uint32_t total;
    uint32_t run = sums[blockIdx.x] + block_scan_256(sum, s, &total);
#pragma unroll
    for (uint32_t k = 0; k < kScanPerThread; ++k) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
}

// ---- stable radix sort: one wave per workgroup, `tile` consecutive elements each ---------------------------------------------
__global__ __launch_bounds__(64) void voxel_sort_count_k(const uint32_t* __restrict__ keys, uint32_t n, uint32_t shift,
                                                         uint32_t tile, uint32_t* __restrict__ counts) {
    __shared__ uint32_t hist[kVoxelSortRadix];
    const uint32_t lane = threadIdx.x;
    for (uint32_t d = lane; d < kVoxelSortRadix; d += 64) hist[d] = 0;
    __syncthreads();
    const size_t beg = (size_t)blockIdx.x * tile;
    const size_t end = beg + tile < n ? beg + tile : n;
    for (size_t k = beg + lane; k < end; k += 64) atomicAdd(&hist[(keys[k] >> shift) & 255u], 1u);
    __syncthreads();
    for (uint32_t d = lane; d < kVoxelSortRadix; d += 64) counts[(size_t)d * gridDim.x + blockIdx.x] = hist[d];
}

__global__ __launch_bounds__(64) void voxel_sort_scatter_k(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in,
                                                           uint32_t n, uint32_t shift, uint32_t tile,
                                                           const uint32_t* __restrict__ counts, uint32_t* __restrict__ keys_out,
                                                           uint32_t* __restrict__ vals_out) {
    __shared__ uint32_t base[kVoxelSortRadix];   // where the workgroup's next element of each digit goes
    const uint32_t lane = threadIdx.x;
    for (uint32_t d = lane; d < kVoxelSortRadix; d += 64) base[d] = counts[(size_t)d * gridDim.x + blockIdx.x];
    __syncthreads();
    const size_t beg = (size_t)blockIdx.x * tile;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t r = 0; r < tile; r += 64) {   // (tile is a multiple of 64: every lane runs every round)
        const size_t k = beg + r + lane;
        const bool valid = k < n;
        const uint32_t key = valid ? keys_in[k] : 0u;
        const uint32_t val = valid ? (vals_in ? vals_in[k] : (uint32_t)k) : 0u;
        const uint32_t d = (key >> shift) & 255u;
        // the lanes of this round that hold the same digit
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(valid && bit);
            peers &= bit ? bal : ~bal;
        }
        uint32_t dst = 0;
        if (valid) dst = base[d] + (uint32_t)__popcll(peers & below);   // earlier lanes first: stable
        __syncthreads();
        if (valid && (peers >> lane) == 1ull) base[d] += (uint32_t)__popcll(peers);   // the highest peer moves the digit on
        __syncthreads();
        if (valid) {
            keys_out[dst] = key;
            vals_out[dst] = val;
        }
    }
}

__global__ __launch_bounds__(256) void voxel_offsets_k(const uint32_t* __restrict__ sorted_keys, uint32_t n, uint32_t m,
                                                       uint32_t* __restrict__ offsets) {
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const uint32_t key = sorted_keys[k];
    if (k == 0 || sorted_keys[k - 1] != key) offsets[key] = (uint32_t)k;
    if (k == 0) offsets[m] = n;
}

// ---- the ordered sums ---------------------------------------------------------------------------------------------------
constexpr uint32_t kMeanStride = 9;   // doubles per staged member: xyz, normal, colour (consecutive lanes, consecutive banks)

__global__ __launch_bounds__(64) void voxel_means_k(const double* __restrict__ xyz, const double* __restrict__ normals,
                                                    const double* __restrict__ colors, const uint32_t* __restrict__ order,
                                                    const uint32_t* __restrict__ offsets, uint32_t m,
                                                    double* __restrict__ out_xyz, double* __restrict__ out_normals,
                                                    double* __restrict__ out_colors) {
    __shared__ double s[64 * kMeanStride];
    __shared__ uint32_t s_skip[64];
    const uint32_t lane = threadIdx.x;
    const uint32_t set = lane / 3, comp = lane % 3;   // lanes 0-2 the point, 3-5 the normal, 6-8 the colour
    const bool adds = set == 0 || (set == 1 && normals) || (set == 2 && colors);
    for (uint32_t j = blockIdx.x; j < m; j += gridDim.x) {
        const uint32_t beg = offsets[j], end = offsets[j + 1];
        double acc = 0.0;
        for (uint32_t b = beg; b < end; b += 64) {
            const uint32_t k = b + lane;
            if (k < end) {
                const size_t i = order ? order[k] : k;
                double* row = s + lane * kMeanStride;
                row[0] = xyz[3 * i];
                row[1] = xyz[3 * i + 1];
                row[2] = xyz[3 * i + 2];
                if (normals) {
                    const double nx = normals[3 * i], ny = normals[3 * i + 1], nz = normals[3 * i + 2];
                    row[3] = nx;
                    row[4] = ny;
                    row[5] = nz;
                    s_skip[lane] = (nx != nx || ny != ny || nz != nz) ? 1u : 0u;   // a NaN component: the normal is not added
                }
                if (colors) {
                    row[6] = colors[3 * i];
                    row[7] = colors[3 * i + 1];
                    row[8] = colors[3 * i + 2];
                }
            }
            __syncthreads();
            const uint32_t cnt = end - b < 64u ? end - b : 64u;
            if (adds) {
                if (set == 1) {
                    for (uint32_t t = 0; t < cnt; ++t)
                        if (!s_skip[t]) acc += s[t * kMeanStride + lane];
                } else {
                    for (uint32_t t = 0; t < cnt; ++t) acc += s[t * kMeanStride + lane];   // ascending index, one rounded add each
                }
            }
            __syncthreads();
        }
        if (adds) {
            const double mean = acc / (double)(end - beg);
            double* out = set == 0 ? out_xyz : (set == 1 ? out_normals : out_colors);
            out[3 * (size_t)j + comp] = mean;
        }
    }
}

inline uint32_t blocks_for(size_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

}  // namespace

size_t voxel_scan_scratch(size_t n) { return (n + kVoxelScanTile - 1) / kVoxelScanTile + 1; }

void launch_scan_exclusive(const uint32_t* in, uint32_t* out, size_t n, uint32_t* scratch, uint32_t* total_dev, hipStream_t st) {
    const size_t nb = (n + kVoxelScanTile - 1) / kVoxelScanTile;
    if (nb) scan_reduce_k<<<(uint32_t)nb, 256, 0, st>>>(in, n, scratch);
    scan_sums_k<<<1, 256, 0, st>>>(scratch, nb, total_dev);
    if (nb) scan_apply_k<<<(uint32_t)nb, 256, 0, st>>>(in, out, n, scratch);
}

void launch_voxel_bounds(const double* xyz, uint32_t n, VoxelBounds* partial, VoxelBounds* out, hipStream_t st) {
    const uint32_t nb = std::min(kVoxelBoundsBlocks, std::max(1u, blocks_for(n, 256)));
    voxel_bounds_k<<<nb, 256, 0, st>>>(xyz, n, partial);
    voxel_bounds_final_k<<<1, 256, 0, st>>>(partial, nb, out);
}

void launch_voxel_keys(const double* xyz, uint32_t n, const VoxelGrid& g, bool wide, unsigned long long* key64,
                       uint32_t* key96, hipStream_t st) {
    if (wide)
        voxel_keys_k<true><<<blocks_for(n, 256), 256, 0, st>>>(xyz, n, g, key64, key96);
    else
        voxel_keys_k<false><<<blocks_for(n, 256), 256, 0, st>>>(xyz, n, g, key64, key96);
}

void launch_voxel_insert(uint32_t n, bool wide, const unsigned long long* key64, const uint32_t* key96,
                         unsigned long long* table64, uint32_t* table32, uint32_t table_size, uint32_t* first,
                         uint32_t* slot_of, hipStream_t st) {
    if (wide)
        voxel_insert_k<true><<<blocks_for(n, 256), 256, 0, st>>>(n, key64, key96, table64, table32, table_size - 1, first, slot_of);
    else
        voxel_insert_k<false><<<blocks_for(n, 256), 256, 0, st>>>(n, key64, key96, table64, table32, table_size - 1, first, slot_of);
}

void launch_voxel_flags(uint32_t n, const uint32_t* slot_of, const uint32_t* first, uint32_t* is_first, hipStream_t st) {
    voxel_flags_k<<<blocks_for(n, 256), 256, 0, st>>>(n, slot_of, first, is_first);
}

void launch_voxel_ids(uint32_t n, const uint32_t* slot_of, const uint32_t* first, const uint32_t* rank, uint32_t* vid,
                      uint32_t* first_index, hipStream_t st) {
    voxel_ids_k<<<blocks_for(n, 256), 256, 0, st>>>(n, slot_of, first, rank, vid, first_index);
}

void voxel_sort_shape(uint32_t n, uint32_t* tile, uint32_t* blocks) {
    uint32_t t = 2048;
    while (blocks_for(n, t) > kVoxelSortMaxBlocks) t *= 2;
    *tile = t;
    *blocks = std::max(1u, blocks_for(n, t));
}

void launch_voxel_sort_count(const uint32_t* keys, uint32_t n, uint32_t shift, uint32_t* counts, hipStream_t st) {
    uint32_t tile, blocks;
    voxel_sort_shape(n, &tile, &blocks);
    voxel_sort_count_k<<<blocks, 64, 0, st>>>(keys, n, shift, tile, counts);
}

void launch_voxel_sort_scatter(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t n, uint32_t shift,
                               const uint32_t* counts, uint32_t* keys_out, uint32_t* vals_out, hipStream_t st) {
    uint32_t tile, blocks;
    voxel_sort_shape(n, &tile, &blocks);
    voxel_sort_scatter_k<<<blocks, 64, 0, st>>>(keys_in, vals_in, n, shift, tile, counts, keys_out, vals_out);
}

void launch_voxel_offsets(const uint32_t* sorted_keys, uint32_t n, uint32_t m, uint32_t* offsets, hipStream_t st) {
    voxel_offsets_k<<<blocks_for(n, 256), 256, 0, st>>>(sorted_keys, n, m, offsets);
}

void launch_voxel_means(const double* xyz, const double* normals, const double* colors, const uint32_t* order,
                        const uint32_t* offsets, uint32_t m, double* out_xyz, double* out_normals, double* out_colors,
                        hipStream_t st) {
    const uint32_t grid = std::min(m, 1u << 16);
    voxel_means_k<<<grid, 64, 0, st>>>(xyz, normals, colors, order, offsets, m, out_xyz, out_normals, out_colors);
}

}  // namespace m3d
