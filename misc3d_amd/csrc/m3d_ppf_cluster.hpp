// m3d_ppf_cluster.hpp -- launchers of the PPF pose clustering kernels (m3d_ppf_cluster.hip), called by m3d_ppf_cluster.cpp, and
// what that file's m3d_ppf_estimate needs of m3d_ppf.cpp: the model's host side and the vote in its two halves.
// The contract is in include/misc3d_amd.h ("PPF pose clustering"), the arithmetic in m3d_ppf_cluster_fp.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/misc3d_amd.h"
#include "m3d_ppf.hpp"
#include "m3d_ppf_cluster_fp.hpp"

struct m3d_ppf_model;

namespace m3d {

struct DeviceCtx;

// ---- the bridge between m3d_ppf.cpp (the model, the vote) and m3d_ppf_cluster.cpp (the estimate)
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

// the caller's arrays as the host drivers pass them on
struct PpfCloud {
    const double *pts, *nrm;   // n x 3 each
    size_t n;
};
struct PpfScene {
    PpfCloud sample;           // the reference points are read from it
    const size_t* reference;   // n_ref indices into the sample
    size_t n_ref;
    const PpfCloud* edges;     // the scene's edge points, which are then the cloud that is scanned; null: SampledPoints
};
struct PpfVoteOut {            // m3d_ppf_vote's result arrays, `capacity` entries each
    size_t capacity;
    size_t* n_maxima;
    uint32_t *ref_pos, *model_index, *alpha_index, *votes;
    double* poses;             // capacity x 16, may be null
};

// One vote between its two halves.  ppf_check_vote is everything that needs no device: the null checks (out: the caller's
// result arrays, null when the caller keeps the maxima itself), the mode of the model against the scene's, ranges, finiteness,
// the reference indices, the scene frames and EdgePoints' gathered reference points.  ppf_vote_on runs the kernel on a lane the
// caller holds and leaves the maxima in ascending (reference position, model index) order; it sets every field of stats but
// ms_total, which is the caller's clock.  ppf_vote_pose: rule V8 for maximum k.
struct PpfVote {
    std::vector<uint32_t> ref;           // n_ref indices into the cloud the kernel reads the reference points from
    std::vector<double> tsg, rows;       // n_ref x 16: the scene frames; n_ref x 8: their rows 1 and 2, as the kernel reads them
    std::vector<double> rpts, rnrm;      // EdgePoints: the reference points alone, gathered in reference order
    std::vector<PpfMaximum> maxima;
    m3d_ppf_vote_stats stats{};
};
int ppf_check_vote(const m3d_ppf_model* h, const PpfScene& scene, const PpfVoteOut* out, PpfVote* V);
int ppf_vote_on(DeviceCtx* held, const m3d_ppf_model* h, const PpfScene& scene, PpfVote* V);
void ppf_vote_pose(const m3d_ppf_model* h, const PpfVote& V, size_t k, double* pose16);

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
