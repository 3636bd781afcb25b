// m3d_ppf_cluster.hpp -- launchers of the PPF pose clustering kernels (m3d_ppf_cluster.hip), called by m3d_ppf_cluster.cpp.
// The contract is in include/misc3d_amd.h ("PPF pose clustering"), the arithmetic in m3d_ppf_cluster_fp.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "m3d_ppf_cluster_fp.hpp"

struct m3d_ppf_model;

namespace m3d {

// what the clustering's driver reads of a trained model (m3d_ppf.cpp)
struct PpfModelHost {
    uint32_t n;
    int device;
    double diameter, dist_step;
    const double* centroid;   // 3
    const double* centred;    // n x 3
    bool edges;               // trained in EdgePoints mode (m3d_ppf_model_create_edges)
};
PpfModelHost ppf_model_host(const m3d_ppf_model* h);

constexpr uint32_t kPcTile = 256;               // threads of a workgroup = poses of a j tile
constexpr uint32_t kPcNone = 0xFFFFFFFFu;       // label of a pose that belongs to no cluster
constexpr uint32_t kPcMaxValid = 1u << 18;      // valid poses of one call (K2's prefix): 124 bytes of scratch each
constexpr uint32_t kPcRows = 12;                // a pose on the device: t (3), then R row-major (9), structure of arrays

// What one level's kernels read and write.  Level 1 relates poses by translation (K3); level 2 by translation and rotation
// and only inside a translation cluster (K5: group[i] == group[j] != kPcNone).
struct PcLevel {
    const double* pose;      // kPcRows x n, pose[k n + i]
    uint32_t n;
    double r2, cos_edge;
    const uint32_t* group;   // level 2: the level-1 labels; level 1: null
    uint32_t* count;         // n, zero on entry: neighbours (itself included)
    uint32_t* max_count;     // level 1: one word; level 2: n words indexed by group label; zero on entry
    uint32_t* core;          // n
    uint32_t* parent;        // n
    uint32_t* label;         // n: the lowest core index of the pose's cluster, or kPcNone
};

// count, max, core, union, flatten, border: six launches on `st`; `splits` workgroups share the j tiles of a row block
void launch_pc_level(const PcLevel& L, int level, uint32_t splits, hipStream_t st);
constexpr uint32_t kPcLaunchesPerLevel = 6, kPcPairKernelsPerLevel = 3;

}  // namespace m3d
