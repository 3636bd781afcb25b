// m3d_knn.hip -- KNearestSearch (src/knn.cpp) on gfx950: the exact k nearest rows of a resident dim x N matrix.
//
// One lane per query.  Each lane keeps its kk smallest (key, index) pairs sorted in LDS, laid out [slot][lane] (as
// boundary_k's lists), and the kk-th pair in registers: a row is offered to the list only when it beats that pair, so
// most rows cost one compare.  Distances are the serial fp64 sum of include/misc3d_amd.h: acc = +0, then
// acc = acc + (q[k] - r[k]) * (q[k] - r[k]) for k = 0 .. dim - 1, every operation rounded (fp contract off).
#include <hip/hip_runtime.h>

#include "m3d_knn.hpp"

#pragma clang fp contract(off)

namespace m3d {

namespace {

__device__ __forceinline__ uint64_t knn_key(double d2) {
    return d2 != d2 ? kKnnNanKey : (uint64_t)__double_as_longlong(d2);
}
__device__ __forceinline__ bool knn_less(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
    return ka < kb || (ka == kb && ia < ib);
}

// The lane's sorted list: lk / li[slot][lane], slot < kk; (kth_k, kth_i) = slot kk - 1.
template <int KCAP>
struct KnnList {
    uint64_t (*lk)[64];
    uint32_t (*li)[64];
    int lane, kk;
    uint64_t kth_k;
    uint32_t kth_i;
    __device__ void init() {
        for (int j = 0; j < kk; ++j) {
            lk[j][lane] = ~0ull;
            li[j][lane] = ~0u;
        }
        kth_k = ~0ull;
        kth_i = ~0u;
    }
    __device__ __forceinline__ void offer(uint64_t key, uint32_t idx) {
        if (!knn_less(key, idx, kth_k, kth_i)) return;
        int j = kk - 1;
        while (j > 0) {
            const uint64_t pk = lk[j - 1][lane];
            const uint32_t pi = li[j - 1][lane];
            if (!knn_less(key, idx, pk, pi)) break;
            lk[j][lane] = pk;
            li[j][lane] = pi;
            --j;
        }
        lk[j][lane] = key;
        li[j][lane] = idx;
        kth_k = lk[kk - 1][lane];
        kth_i = li[kk - 1][lane];
    }
};

// ---- tile: brute force, data rows staged through LDS ----------------------------------------------------------------
// grid (ceil(mc / 64), S), 64 lanes: lane = query blockIdx.x 64 + lane, split = blockIdx.y.  The workgroup stages
// kKnnTileRows rows x kKnnTileDims dimensions of its split at a time; every lane reads the same LDS word (broadcast)
// and keeps one accumulator per staged row, so each row's sum still runs in dimension order across the dimension tiles.
template <int KCAP>
__global__ __launch_bounds__(64) void knn_tile_k(const double* __restrict__ data, uint32_t n, int dim,
                                                 const double* __restrict__ qT, uint32_t mc, int kk, uint32_t rows_per_split,
                                                 const uint64_t* __restrict__ floor, uint64_t* __restrict__ part_key,
                                                 uint32_t* __restrict__ part_idx) {
    __shared__ uint64_t lk[KCAP][64];
    __shared__ uint32_t li[KCAP][64];
    __shared__ double tile[kKnnTileRows][kKnnTileDims];
    const int lane = threadIdx.x;
    const uint32_t q = blockIdx.x * 64u + lane;
    const bool live = q < mc;
    const uint32_t s = blockIdx.y, S = gridDim.y;
    const uint64_t r0_ = (uint64_t)s * rows_per_split;
    const uint32_t r0 = (uint32_t)(r0_ < n ? r0_ : n);
    const uint32_t r1 = (uint32_t)(r0_ + rows_per_split < n ? r0_ + rows_per_split : n);
    KnnList<KCAP> L{lk, li, lane, kk, 0, 0};
    L.init();
    uint64_t fk = 0;
    uint32_t fi = 0;
    const bool use_floor = floor != nullptr && live;
    if (use_floor) {
        fk = floor[2 * (size_t)q];
        fi = (uint32_t)floor[2 * (size_t)q + 1];
    }
    for (uint32_t base = r0; base < r1; base += kKnnTileRows) {
        const uint32_t rows = (r1 - base) < (uint32_t)kKnnTileRows ? (r1 - base) : (uint32_t)kKnnTileRows;
        double acc[kKnnTileRows];
#pragma unroll
        for (int t = 0; t < kKnnTileRows; ++t) acc[t] = 0.0;
        for (int k0 = 0; k0 < dim; k0 += kKnnTileDims) {
            const int dc = dim - k0 < kKnnTileDims ? dim - k0 : kKnnTileDims;
            __syncthreads();   // the previous tile's readers are done
            for (int i = lane; i < (int)rows * dc; i += 64) {
                const int t = i / dc, k = i - t * dc;
                tile[t][k] = data[(size_t)(base + t) * dim + k0 + k];
            }
            __syncthreads();
            if (live) {
                for (int k = 0; k < dc; ++k) {
                    const double qk = qT[(size_t)(k0 + k) * mc + q];
#pragma unroll
                    for (int t = 0; t < kKnnTileRows; ++t) {
                        const double d = qk - tile[t][k];   // (rows >= `rows` hold stale values: never offered)
                        acc[t] = acc[t] + d * d;
                    }
                }
            }
        }
        if (live) {
#pragma unroll
            for (int t = 0; t < kKnnTileRows; ++t) {
                if ((uint32_t)t < rows) {
                    const uint64_t key = knn_key(acc[t]);
                    const uint32_t idx = base + t;
                    if (!use_floor || knn_less(fk, fi, key, idx)) L.offer(key, idx);
                }
            }
        }
    }
    if (live) {
        const size_t out = ((size_t)q * S + s) * kk;
        for (int j = 0; j < kk; ++j) {
            part_key[out + j] = lk[j][lane];
            part_idx[out + j] = li[j][lane];
        }
    }
}

__device__ __forceinline__ void knn_shfl_min(uint64_t& k, uint32_t& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)k, off, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), off, 64);
        const uint32_t oi = (uint32_t)__shfl_xor((int)i, off, 64);
        const uint64_t ok = ((uint64_t)hi << 32) | lo;
        if (knn_less(ok, oi, k, i)) {
            k = ok;
            i = oi;
        }
    }
}

// ---- merge: one wavefront per query, lane l owns lists l, l + 64, l + 128, l + 192 ----------------------------------
__global__ __launch_bounds__(256) void knn_merge_k(const uint64_t* __restrict__ part_key,
                                                   const uint32_t* __restrict__ part_idx, uint32_t mc, int kk, int S,
                                                   uint64_t* __restrict__ floor, double* __restrict__ out_d2,
                                                   uint32_t* __restrict__ out_idx) {
    const int lane = threadIdx.x & 63;
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= mc) return;   // (uniform per wavefront)
    const size_t base = (size_t)q * S * kk;
    int pos[4] = {0, 0, 0, 0};
    for (int o = 0; o < kk; ++o) {
        uint64_t bk = ~0ull;
        uint32_t bi = ~0u;
        int bj = -1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int s = lane + 64 * j;
            if (s < S && pos[j] < kk) {
                const size_t at = base + (size_t)s * kk + pos[j];
                const uint64_t k = part_key[at];
                const uint32_t i = part_idx[at];
                if (knn_less(k, i, bk, bi)) {
                    bk = k;
                    bi = i;
                    bj = j;
                }
            }
        }
        uint64_t mk = bk;
        uint32_t mi = bi;
        knn_shfl_min(mk, mi);
        if (bj >= 0 && bk == mk && bi == mi) {   // the owner of the smallest head (pairs are distinct) advances
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j == bj) ++pos[j];
        }
        if (lane == 0) {
            out_d2[(size_t)q * kk + o] = __longlong_as_double((long long)mk);
            out_idx[(size_t)q * kk + o] = mi;
            if (floor && o == kk - 1) {
                floor[2 * (size_t)q] = mk;
                floor[2 * (size_t)q + 1] = mi;
            }
        }
    }
}

// ---- grid (dim 3) ----------------------------------------------------------------------------------------------------
// Shell r visits the cells at Chebyshev distance r from the query's cell cq (clamped to [-1, n_a] per axis; any cq is
// correct, a near one is fast).  After shells 0 .. r every unvisited grid row p lies in a cell outside the block
// [cq - r, cq + r]^3, so on some axis a its cell index c is <= cq_a - r - 1 or >= cq_a + r + 1.
//   Low side: p_a <= P := pmax[a][cq_a - r - 1], so q_a - p_a >= q_a - P as reals, and rounding is monotone:
//   |fl(q_a - p_a)| >= g := fl(q_a - P).  If g > 0 then fl(d * d) >= fl(g * g) (monotone again), and the serial sum of
//   non-negative rounded terms never decreases: fl(acc + t) >= fl(0 + t) = t for acc >= 0, and later terms only add.
//   So computed d2(p) >= B_a := fl(g * g).  The high side is the same with g := fl(smin[a][cq_a + r + 1] - q_a)
//   (fl(p - q) = -fl(q - p) exactly).  A side with no cells contributes no row (B = +inf); g <= 0 gives B = 0.
// So every unvisited grid row has key >= key(B), B = the minimum over the six sides, and once the kk-th pair's key is
// strictly below key(B) no unvisited row can enter the list (its pair is larger whatever its index): the list is final.
// The search also ends when the block covers the grid.  It never relies on where the query's cell "really" is, nor on
// how the host rounded the rows into cells: P and the suffix minima are the rows' own coordinates.
template <int KCAP>
__global__ __launch_bounds__(64) void knn_grid_k(KnnGridView v, const double* __restrict__ q3, uint32_t mc, int kk,
                                                 double* __restrict__ out_d2, uint32_t* __restrict__ out_idx,
                                                 unsigned long long* __restrict__ pairs_seen) {
    __shared__ uint64_t lk[KCAP][64];
    __shared__ uint32_t li[KCAP][64];
    const int lane = threadIdx.x;
    const uint32_t q = blockIdx.x * 64u + lane;
    if (q >= mc) return;   // (no barrier below)
    KnnList<KCAP> L{lk, li, lane, kk, 0, 0};
    L.init();
    const KnnGridDesc& g = v.g;
    const double qa[3] = {q3[3 * (size_t)q], q3[3 * (size_t)q + 1], q3[3 * (size_t)q + 2]};
    const double oa[3] = {g.ox, g.oy, g.oz};
    const int na[3] = {g.nx, g.ny, g.nz};
    int cq[3];
    for (int a = 0; a < 3; ++a) {
        const double c = floor((qa[a] - oa[a]) * g.inv_h);
        cq[a] = c < -1.0 ? -1 : (c > (double)na[a] ? na[a] : (int)c);
    }
    unsigned long long seen = 0;
    for (int r = 0;; ++r) {
        const int z0 = -r > -cq[2] ? -r : -cq[2], z1 = r < g.nz - 1 - cq[2] ? r : g.nz - 1 - cq[2];
        const int y0 = -r > -cq[1] ? -r : -cq[1], y1 = r < g.ny - 1 - cq[1] ? r : g.ny - 1 - cq[1];
        const int x0 = -r > -cq[0] ? -r : -cq[0], x1 = r < g.nx - 1 - cq[0] ? r : g.nx - 1 - cq[0];
        for (int dz = z0; dz <= z1; ++dz) {
            for (int dy = y0; dy <= y1; ++dy) {
                const bool face = dz == -r || dz == r || dy == -r || dy == r;
                for (int dx = face ? x0 : -r; dx <= (face ? x1 : r); dx += face || r == 0 ? 1 : 2 * r) {
                    if (dx < x0 || dx > x1) continue;
                    const uint32_t c = ((uint32_t)(cq[2] + dz) * (uint32_t)g.ny + (uint32_t)(cq[1] + dy)) * (uint32_t)g.nx +
                                       (uint32_t)(cq[0] + dx);
                    const uint32_t e = v.cell_start[c + 1];
                    for (uint32_t p = v.cell_start[c]; p < e; ++p) {
                        const double ex = qa[0] - v.sx[p], ey = qa[1] - v.sy[p], ez = qa[2] - v.sz[p];
                        double acc = 0.0;
                        acc = acc + ex * ex;
                        acc = acc + ey * ey;
                        acc = acc + ez * ez;
                        L.offer(knn_key(acc), v.sidx[p]);
                    }
                    seen += e - v.cell_start[c];
                }
            }
        }
        bool covered = true;
        double B = __builtin_inf();
        for (int a = 0; a < 3; ++a) {
            const int lo = cq[a] - r - 1, hi = cq[a] + r + 1;
            if (lo >= 0) {
                covered = false;
                const double gap = qa[a] - v.pmax[a][lo < na[a] ? lo : na[a] - 1];
                const double b = gap > 0.0 ? gap * gap : 0.0;
                B = b < B ? b : B;
            }
            if (hi < na[a]) {
                covered = false;
                const double gap = v.smin[a][hi > 0 ? hi : 0] - qa[a];
                const double b = gap > 0.0 ? gap * gap : 0.0;
                B = b < B ? b : B;
            }
        }
        if (covered || L.kth_k < knn_key(B)) break;
    }
    for (uint32_t t = 0; t < g.n_out; ++t) {   // rows with a non-finite coordinate: d2 is +inf or NaN
        const uint32_t row = v.out_rows[t];
        const double* p = v.data + 3 * (size_t)row;
        const double ex = qa[0] - p[0], ey = qa[1] - p[1], ez = qa[2] - p[2];
        double acc = 0.0;
        acc = acc + ex * ex;
        acc = acc + ey * ey;
        acc = acc + ez * ez;
        L.offer(knn_key(acc), row);
    }
    seen += g.n_out;
    for (int j = 0; j < kk; ++j) {
        out_d2[(size_t)q * kk + j] = __longlong_as_double((long long)lk[j][lane]);
        out_idx[(size_t)q * kk + j] = li[j][lane];
    }
    atomicAdd(pairs_seen, seen);
}

}  // namespace

void launch_knn_tile(const double* data, uint32_t n, int dim, const double* qT, uint32_t mc, int kk, int splits,
                     uint32_t rows_per_split, const uint64_t* floor, uint64_t* part_key, uint32_t* part_idx, hipStream_t st) {
    if (!mc || kk <= 0) return;
    const dim3 grid((mc + 63) / 64, (unsigned)splits);
#define M3D_KNN_TILE(C) knn_tile_k<C><<<grid, 64, 0, st>>>(data, n, dim, qT, mc, kk, rows_per_split, floor, part_key, part_idx)
    if (kk <= 16)
        M3D_KNN_TILE(16);
    else if (kk <= 32)
        M3D_KNN_TILE(32);
    else if (kk <= 64)
        M3D_KNN_TILE(64);
    else
        M3D_KNN_TILE(128);
#undef M3D_KNN_TILE
}

void launch_knn_merge(const uint64_t* part_key, const uint32_t* part_idx, uint32_t mc, int kk, int splits, uint64_t* floor,
                      double* out_d2, uint32_t* out_idx, hipStream_t st) {
    if (!mc || kk <= 0) return;
    knn_merge_k<<<(mc + 3) / 4, 256, 0, st>>>(part_key, part_idx, mc, kk, splits, floor, out_d2, out_idx);
}

void launch_knn_grid(const KnnGridView& v, const double* q3, uint32_t mc, int kk, double* out_d2, uint32_t* out_idx,
                     unsigned long long* pairs_seen, hipStream_t st) {
    if (!mc || kk <= 0) return;
    const unsigned blocks = (mc + 63) / 64;
#define M3D_KNN_GRID(C) knn_grid_k<C><<<blocks, 64, 0, st>>>(v, q3, mc, kk, out_d2, out_idx, pairs_seen)
    if (kk <= 16)
        M3D_KNN_GRID(16);
    else if (kk <= 32)
        M3D_KNN_GRID(32);
    else if (kk <= 64)
        M3D_KNN_GRID(64);
    else
        M3D_KNN_GRID(128);
#undef M3D_KNN_GRID
}

}  // namespace m3d
