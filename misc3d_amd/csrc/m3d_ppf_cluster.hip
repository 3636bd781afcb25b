// m3d_ppf_cluster.hip -- the pose clustering of PPFEstimator (ClusterPoses / GatherPose / CalcPoseNeighbor,
// src/ppf_estimation.cpp:778-935) on gfx950, restated without the reference's stack (include/misc3d_amd.h, "PPF pose
// clustering", K3 - K5): neighbour counts, cores, the connected components of the cores, and the border poses' clusters.
//
// Every pair kernel is the same tiled all-pairs loop: a thread per pose i, the j side staged through LDS in tiles of 256 as
// structure-of-arrays doubles (3 per pose at level 1, 12 at level 2: 24 KiB), every lane of a wave reading the same j -- an
// LDS broadcast.  blockIdx.y splits the j tiles of a row block over workgroups when the row blocks alone would not fill the
// device.  Every output is an integer and none depends on the split or on scheduling: counts are added atomically, the
// largest count is an atomic max, a component's root is its lowest member whatever the order of the hooks
// (m3d_union_find.hpp), and a border pose takes the minimum root over its core neighbours by an atomic min.
#include <hip/hip_runtime.h>

#include "m3d_ppf_cluster.hpp"
#include "m3d_union_find.hpp"

#pragma clang fp contract(off)

namespace m3d {

namespace {

template <int Level>
struct PcTileLds {
    double v[Level == 1 ? 3 : kPcRows][kPcTile];
    uint32_t group[kPcTile];
    uint32_t aux[kPcTile];
};

// visit(j, aux[j]) for every j of this workgroup's tiles that matches pose i = blockIdx.x * 256 + threadIdx.x (i itself is
// one).  aux_of(j) is staged beside the tile.  Every thread of the workgroup must call it (barriers).
template <int Level, class Aux, class Visit>
__device__ __forceinline__ void pc_pair_loop(const PcLevel& L, PcTileLds<Level>& S, Aux aux_of, Visit visit) {
    constexpr int kRows = Level == 1 ? 3 : (int)kPcRows;
    const uint32_t n = L.n, tid = threadIdx.x;
    const uint32_t i = blockIdx.x * kPcTile + tid;
    const bool live = i < n;
    double mine[kRows];
#pragma unroll
    for (int k = 0; k < kRows; ++k) mine[k] = live ? L.pose[(size_t)k * n + i] : 0.0;
    const uint32_t my_group = (Level == 2 && live) ? L.group[i] : 0u;
    const bool active = live && (Level == 1 || my_group != kPcNone);
    const uint32_t n_tiles = (n + kPcTile - 1) / kPcTile;
    for (uint32_t tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        const uint32_t j0 = tile * kPcTile;
        const uint32_t nj = n - j0 < kPcTile ? n - j0 : kPcTile;
        __syncthreads();
        if (tid < nj) {
            const uint32_t j = j0 + tid;
#pragma unroll
            for (int k = 0; k < kRows; ++k) S.v[k][tid] = L.pose[(size_t)k * n + j];
            if constexpr (Level == 2) S.group[tid] = L.group[j];
            S.aux[tid] = aux_of(j);
        }
        __syncthreads();
        if (!active) continue;
        for (uint32_t u = 0; u < nj; ++u) {
            const double d2 = pc_d2(S.v[0][u] - mine[0], S.v[1][u] - mine[1], S.v[2][u] - mine[2]);
            bool m = pc_match_t(d2, L.r2);
            if constexpr (Level == 2) {
                m = m && S.group[u] == my_group;
                if (m) {
                    double theirs[9];
#pragma unroll
                    for (int k = 0; k < 9; ++k) theirs[k] = S.v[3 + k][u];
                    m = pc_match_tr(d2, L.r2, pc_ca(pc_trace(&mine[kRows - 9], theirs)), L.cos_edge);
                }
            }
            if (m) visit(j0 + u, S.aux[u]);
        }
    }
}

template <int Level>
__global__ __launch_bounds__(256) void pc_count_k(PcLevel L) {
    __shared__ PcTileLds<Level> S;
    uint32_t c = 0;
    pc_pair_loop<Level>(L, S, [](uint32_t) { return 0u; }, [&](uint32_t, uint32_t) { ++c; });
    const uint32_t i = blockIdx.x * kPcTile + threadIdx.x;
    if (i < L.n && c) atomicAdd(L.count + i, c);
}

// the largest count: of all poses (level 1, one word) or per translation cluster (level 2, the word of its label).  Counts up
// to 6 change nothing (pc_min_num_pt) and are not sent.
__global__ __launch_bounds__(256) void pc_max_k(PcLevel L) {
    __shared__ uint32_t block_max;
    const uint32_t i = blockIdx.x * kPcTile + threadIdx.x;
    const uint32_t c = i < L.n ? L.count[i] : 0u;
    if (L.group) {
        if (i < L.n && c > 6u && L.group[i] != kPcNone) atomicMax(L.max_count + L.group[i], c);
        return;
    }
    if (threadIdx.x == 0) block_max = 0;
    __syncthreads();
    if (c > 6u) atomicMax(&block_max, c);
    __syncthreads();
    if (threadIdx.x == 0 && block_max) atomicMax(L.max_count, block_max);
}

__global__ __launch_bounds__(256) void pc_core_k(PcLevel L) {
    const uint32_t i = blockIdx.x * kPcTile + threadIdx.x;
    if (i >= L.n) return;
    const uint32_t g = L.group ? L.group[i] : 0u;
    const bool in = g != kPcNone;
    L.core[i] = (in && L.count[i] >= pc_min_num_pt(L.max_count[g])) ? 1u : 0u;
    L.parent[i] = i;
}

template <int Level>
__global__ __launch_bounds__(256) void pc_union_k(PcLevel L) {
    __shared__ PcTileLds<Level> S;
    const uint32_t i = blockIdx.x * kPcTile + threadIdx.x;
    const bool core_i = i < L.n && L.core[i] != 0u;
    const uint32_t* core = L.core;
    uint32_t* parent = L.parent;
    pc_pair_loop<Level>(L, S, [core](uint32_t j) { return core[j]; }, [&](uint32_t j, uint32_t core_j) {
        if (core_i && core_j && j < i) uf_unite(parent, j, i);   // every unordered pair once
    });
}

// after the union launch has ended: plain loads
__global__ __launch_bounds__(256) void pc_flatten_k(PcLevel L) {
    const uint32_t i = blockIdx.x * kPcTile + threadIdx.x;
    if (i >= L.n) return;
    uint32_t x = kPcNone;
    if (L.core[i]) {
        x = i;
        for (uint32_t p = L.parent[x]; p != x; p = L.parent[x]) x = p;
    }
    L.label[i] = x;
}

// a pose that is no core joins the cluster with the lowest root among its core neighbours.  label[] of a core is final here
// and is the only thing read; label[] of a non-core is the only thing written.
template <int Level>
__global__ __launch_bounds__(256) void pc_border_k(PcLevel L) {
    __shared__ PcTileLds<Level> S;
    const uint32_t i = blockIdx.x * kPcTile + threadIdx.x;
    const bool border_i = i < L.n && L.core[i] == 0u;
    const uint32_t* core = L.core;
    const uint32_t* label = L.label;
    uint32_t best = kPcNone;
    pc_pair_loop<Level>(L, S, [core, label](uint32_t j) { return core[j] ? label[j] : kPcNone; }, [&](uint32_t, uint32_t root_j) {
        if (root_j < best) best = root_j;
    });
    if (border_i && best != kPcNone) atomicMin(L.label + i, best);
}

template <int Level>
void launch_level(const PcLevel& L, uint32_t splits, hipStream_t st) {
    const uint32_t rows = (L.n + kPcTile - 1) / kPcTile;
    const dim3 pair_grid(rows, splits), flat_grid(rows);
    pc_count_k<Level><<<pair_grid, kPcTile, 0, st>>>(L);
    pc_max_k<<<flat_grid, kPcTile, 0, st>>>(L);
    pc_core_k<<<flat_grid, kPcTile, 0, st>>>(L);
    pc_union_k<Level><<<pair_grid, kPcTile, 0, st>>>(L);
    pc_flatten_k<<<flat_grid, kPcTile, 0, st>>>(L);
    pc_border_k<Level><<<pair_grid, kPcTile, 0, st>>>(L);
}

}  // namespace

void launch_pc_level(const PcLevel& L, int level, uint32_t splits, hipStream_t st) {
    if (L.n == 0) return;
    const uint32_t rows = (L.n + kPcTile - 1) / kPcTile;
    if (splits < 1) splits = 1;
    if (splits > rows) splits = rows;   // (as many j tiles as row blocks)
    if (level == 1)
        launch_level<1>(L, splits, st);
    else
        launch_level<2>(L, splits, st);
}

}  // namespace m3d
