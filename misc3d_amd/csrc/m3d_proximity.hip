// m3d_proximity.hip -- ProximityExtractor (src/proximity_extraction.cpp) on gfx950: the clusters are the connected
// components of the graph "j in the radius neighbourhood of i and evaluator(i, j, dist)" ("Proximity
// extraction"), found with a lock-free union-find over original point indices.
//
// The union-find (uf_find, uf_unite), its parent[] invariant and its coherence argument are in m3d_union_find.hpp; the
// flatten kernel runs after the union launch has ended and reads with plain loads.  The scan of a point's 3x3x3 block
// (prox_scan_block) is m3d_prox_scan.hpp's.
#include <hip/hip_runtime.h>

#include "m3d_prox_scan.hpp"
#include "m3d_proximity.hpp"
#include "m3d_union_find.hpp"

#pragma clang fp contract(off)

namespace m3d {

namespace {

__global__ void prox_init_k(uint32_t* __restrict__ parent, uint32_t* __restrict__ size, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    parent[i] = i;
    size[i] = 0;
}

__global__ void prox_gather_normals_k(CloudView c, const uint32_t* __restrict__ cell_orig, const uint32_t* __restrict__ n_sorted,
                                      double* __restrict__ snx, double* __restrict__ sny, double* __restrict__ snz) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_sorted[0]) return;
    const uint32_t i = cell_orig[t];
    snx[t] = c.nx[i];
    sny[t] = c.ny[i];
    snz[t] = c.nz[i];
}

// one lane per point in grid order: the lanes of a wave share cells and scan the same rows
__global__ __launch_bounds__(256) void prox_union_grid_k(GridDesc g, const uint32_t* __restrict__ cell_start,
                                                         const double* __restrict__ qx, const double* __restrict__ qy,
                                                         const double* __restrict__ qz,
                                                         const uint32_t* __restrict__ cell_orig,
                                                         const double* __restrict__ snx, const double* __restrict__ sny,
                                                         const double* __restrict__ snz,
                                                         const uint32_t* __restrict__ n_sorted, ProxCut cut,
                                                         uint32_t* parent) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_sorted[0]) return;
    const uint32_t i = cell_orig[t];
    const bool normals = cut.kind != kProxDistance;
    const double ax = normals ? snx[t] : 0.0, ay = normals ? sny[t] : 0.0, az = normals ? snz[t] : 0.0;
    prox_scan_block(g, cell_start, qx, qy, qz, t, [&](uint32_t u, double d2) {
        const uint32_t j = cell_orig[u];
        if (j <= i) return;   // every unordered pair once (both built-in evaluators are symmetric)
        const double dot = normals ? dot3(ax, ay, az, snx[u], sny[u], snz[u]) : 0.0;
        if (prox_accept(cut, d2, dot)) uf_unite(parent, i, j);
    });
}

__global__ __launch_bounds__(256) void prox_union_lists_k(CloudView c, const uint64_t* __restrict__ off,
                                                          const uint32_t* __restrict__ idx, uint32_t n, ProxCut cut,
                                                          uint32_t* parent) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const bool normals = cut.kind != kProxDistance;
    const double px = c.x[i], py = c.y[i], pz = c.z[i];
    const double ax = normals ? c.nx[i] : 0.0, ay = normals ? c.ny[i] : 0.0, az = normals ? c.nz[i] : 0.0;
    const uint64_t e = off[i + 1];
    for (uint64_t k = off[i] + 1; k < e; ++k) {   // j = 1: entry 0 is skipped
        const uint32_t j = idx[k];
        if (j == i) continue;
        const double dx = px - c.x[j], dy = py - c.y[j], dz = pz - c.z[j];
        const double d2 = dot3(dx, dy, dz, dx, dy, dz);   // (p_i - p_j).norm() before its sqrt
        const double dot = normals ? dot3(ax, ay, az, c.nx[j], c.ny[j], c.nz[j]) : 0.0;
        if (prox_accept(cut, d2, dot)) uf_unite(parent, i, j);
    }
}

__global__ void prox_flatten_k(const uint32_t* __restrict__ parent, uint32_t* __restrict__ root, uint32_t* size, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t x = i;
    for (uint32_t p = parent[x]; p != x; p = parent[x]) x = p;
    root[i] = x;
    atomicAdd(size + x, 1u);
}

__global__ __launch_bounds__(256) void prox_nb_count_k(GridDesc g, const uint32_t* __restrict__ cell_start,
                                                       const double* __restrict__ qx, const double* __restrict__ qy,
                                                       const double* __restrict__ qz, const uint32_t* __restrict__ cell_orig,
                                                       const uint32_t* __restrict__ n_sorted, uint32_t* __restrict__ count) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_sorted[0]) return;
    uint32_t m = 0;
    prox_scan_block(g, cell_start, qx, qy, qz, t, [&](uint32_t u, double) { m += u != t; });
    count[cell_orig[t]] = m;
}

__global__ __launch_bounds__(256) void prox_nb_fill_k(GridDesc g, const uint32_t* __restrict__ cell_start,
                                                      const double* __restrict__ qx, const double* __restrict__ qy,
                                                      const double* __restrict__ qz, const uint32_t* __restrict__ cell_orig,
                                                      const uint32_t* __restrict__ n_sorted, const uint64_t* __restrict__ off,
                                                      uint32_t* __restrict__ nb_idx, double* __restrict__ nb_d2) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_sorted[0]) return;
    const uint32_t i = cell_orig[t];
    const uint64_t b = off[i], cap = off[i + 1] - b;
    uint64_t m = 0;
    prox_scan_block(g, cell_start, qx, qy, qz, t, [&](uint32_t u, double d2) {
        if (u == t || m >= cap) return;
        const uint32_t j = cell_orig[u];
        uint64_t pos = m++;   // insertion by (d2, index)
        while (pos > 0 && (d2 < nb_d2[b + pos - 1] || (d2 == nb_d2[b + pos - 1] && j < nb_idx[b + pos - 1]))) {
            nb_d2[b + pos] = nb_d2[b + pos - 1];
            nb_idx[b + pos] = nb_idx[b + pos - 1];
            --pos;
        }
        nb_d2[b + pos] = d2;
        nb_idx[b + pos] = j;
    });
}

inline uint32_t blocks(uint32_t n) { return (n + 255) / 256; }

}  // namespace

void launch_prox_init(uint32_t* parent, uint32_t* size, uint32_t n, hipStream_t st) {
    if (n) prox_init_k<<<blocks(n), 256, 0, st>>>(parent, size, n);
}
void launch_prox_gather_normals(const CloudView& c, const uint32_t* cell_orig, uint32_t n, const uint32_t* n_sorted,
                                double* snx, double* sny, double* snz, hipStream_t st) {
    if (n) prox_gather_normals_k<<<blocks(n), 256, 0, st>>>(c, cell_orig, n_sorted, snx, sny, snz);
}
void launch_prox_union_grid(const GridDesc& g, const uint32_t* cell_start, const double* qx, const double* qy,
                            const double* qz, const uint32_t* cell_orig, const double* snx, const double* sny,
                            const double* snz, uint32_t n, const uint32_t* n_sorted, const ProxCut& cut, uint32_t* parent,
                            hipStream_t st) {
    if (n)
        prox_union_grid_k<<<blocks(n), 256, 0, st>>>(g, cell_start, qx, qy, qz, cell_orig, snx, sny, snz, n_sorted, cut,
                                                      parent);
}
void launch_prox_union_lists(const CloudView& c, const uint64_t* off, const uint32_t* idx, uint32_t n, const ProxCut& cut,
                             uint32_t* parent, hipStream_t st) {
    if (n) prox_union_lists_k<<<blocks(n), 256, 0, st>>>(c, off, idx, n, cut, parent);
}
void launch_prox_flatten(const uint32_t* parent, uint32_t* root, uint32_t* size, uint32_t n, hipStream_t st) {
    if (n) prox_flatten_k<<<blocks(n), 256, 0, st>>>(parent, root, size, n);
}
void launch_prox_nb_count(const GridDesc& g, const uint32_t* cell_start, const double* qx, const double* qy, const double* qz,
                          const uint32_t* cell_orig, uint32_t n, const uint32_t* n_sorted, uint32_t* count, hipStream_t st) {
    if (n) prox_nb_count_k<<<blocks(n), 256, 0, st>>>(g, cell_start, qx, qy, qz, cell_orig, n_sorted, count);
}
void launch_prox_nb_fill(const GridDesc& g, const uint32_t* cell_start, const double* qx, const double* qy, const double* qz,
                         const uint32_t* cell_orig, uint32_t n, const uint32_t* n_sorted, const uint64_t* off,
                         uint32_t* nb_idx, double* nb_d2, hipStream_t st) {
    if (n) prox_nb_fill_k<<<blocks(n), 256, 0, st>>>(g, cell_start, qx, qy, qz, cell_orig, n_sorted, off, nb_idx, nb_d2);
}

}  // namespace m3d
