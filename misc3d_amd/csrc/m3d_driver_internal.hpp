// m3d_driver_internal.hpp -- what the translation units of the host driver share (m3d_device.cpp: errors, lanes, block
// pools, resident clouds; m3d_fit.cpp: the RANSAC loop; m3d_refine.cpp: RefineModel; m3d_segmentation.cpp:
// SegmentPlaneIterative; m3d_multi.cpp: one process, several devices; m3d_bench_hooks.cpp; m3d_preprocessing.cpp, m3d_proximity.cpp,
// m3d_knn.cpp, m3d_fpfh.cpp, m3d_voxel.cpp: the entry points on top).  Not part of any boundary.  The early-return macros, round_up,
// now_ms and stream_wait_spin come from m3d_host_util.hpp, which m3d_registration.cpp, m3d_match.cpp,
// m3d_global_registration.cpp and m3d_normals.hip include on its own; the grid arithmetic from m3d_grid_geom.hpp.
#pragma once
#include "m3d_driver.hpp"
#include "m3d_comm.hpp"
#include "m3d_config.hpp"
#include "m3d_fp.hpp"
#include "m3d_grid_geom.hpp"
#include "m3d_host_util.hpp"
#include "m3d_mt19937.hpp"
#include "m3d_reg_kernels.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <random>
#include <thread>

namespace m3d {

static inline int minimal_sample(int kind) { return kind == M3D_PLANE ? 3 : (kind == M3D_SPHERE ? 4 : 2); }
static inline int num_params(int kind) { return kind == M3D_CYLINDER ? 7 : 4; }

// ---- m3d_device.cpp
const std::string& last_error_string();
bool is_library_pinned(const void* p, size_t bytes);   // inside a block m3d_host_alloc handed out?
void release_buffers(m3d_cloud* c);                    // every device buffer a cloud owns -> its lane's free list

// ---- the state of a fit that is not a lane's (DeviceCtx holds resources only), by lifetime
// What outlives a ROUND of m3d_segment_plane_iterative: owned by segment_impl's stack frame, reached through FitCaller::rounds.
struct SegmentRounds {
    // Deferred RefineModel (one GPU): a round whose early compaction ran on the hypothesis the replay then named does not wait
    // for it -- the inlier count is the scoring pass's, the index list goes to the caller's pinned array by itself -- and its
    // GeneralFit is finished from the pinned sums while the NEXT round's records are awaited (finalize_deferred_refine).  Two
    // slots of h_best / h_moments / the total word, toggled per fit: the next round's compaction is queued before that.
    struct Deferred {
        bool pending = false;
        int slot = 0;
        uint32_t ni = 0;
        double* params_out = nullptr;
    } deferred;
    int slot = 0;
    // a tombstone pass that waits for the next fit's minimal_fit_k launch to ride in (cloud_remove_issue -> issue_chunk)
    bool poison_pending = false;
    PoisonJob pending_poison;
    uint64_t* poison_expected_at = nullptr, poison_pending_count = 0;   // m3d_cloud::Work::poison_expected, credited at launch
    bool spec_hit = false;   // the last fit's early compaction ran on the hypothesis the replay named (cloud_fit_locked)
};
// What the caller of ONE fit asks for (cloud_fit_locked; null: a plain fit).  segment_impl builds one per round.
struct FitCaller {
    // asked right before RefineModel's compaction is queued -- given the inlier count the scoring pass reported (-2: not known
    // yet, -3: the early compaction has been queued), where should the partition of the NON-inliers go (null: none)?
    const std::function<const PartitionOut*(int64_t)>* partition_hook = nullptr;
    // work to queue behind RefineModel's kernels before the host waits for them (the removal of these very inliers)
    const std::function<int(int64_t)>* before_refine_wait = nullptr;
    // rounds on a large part of the cloud: the inlier list (megabytes) is written to this device address (the cluster's slice of
    // a per-call buffer) and shipped by the copy engine under the rounds that follow, instead of being stored over the host link
    // by the compaction kernel itself (which then runs at the link's rate: 370 us for 2.5 M indices) ...
    uint64_t* idx_dev = nullptr;
    bool defer_copy_sync = false;   // ... and the copy stream is waited for once, by the caller, at the end
    bool no_prune_hint = false;     // the fit's chunk will prune nothing (no lead pass, no keep masks)
    bool defer_refine = false;      // RefineModel may finish a round late (SegmentRounds::deferred; needs `rounds`)
    size_t iterations_hint = 0;     // in: iterations of a similar fit, out: of this one
    SegmentRounds* rounds = nullptr;
    const double* best_dev = nullptr;   // out: device address of the fit's best minimal model (a slot's params or best_params)
};
// What is known of a queued RefineModel compaction (issue_refine_compaction fills it; empty: none queued)
struct Compaction {
    const void* total = nullptr;    // pinned: where its inlier total arrives
    bool early = false;             // queued on the device's own pick, before the replay (run_ransac)
    bool fused = false;             // it carried the moments
    uint64_t* idx_host = nullptr;   // ... and wrote the index list to this page-locked destination as well
    // ... or (m3d_config.list_mask) shipped the inliers as a bit mask + per-tile counts, which refine() expands into idx_host
    // after its wait; the device list is not written.  mask_early: "mask ready" (h_sync word 2) comes before the moments' fold
    bool mask = false, mask_early = false;
    bool ev_recorded = false;       // ev_compact was recorded right behind it (a removal has been queued after it)
};
// the pinned words RefineModel's kernels write, per slot (a round that may be finished late; slot 0 otherwise)
inline int refine_slot(const FitCaller* fc) { return fc && fc->defer_refine ? fc->rounds->slot : 0; }
inline double* h_best_at(DeviceCtx* ctx, int slot) { return ctx->h_best.as<double>() + (size_t)slot * kModelStride; }
inline uint8_t* h_total_at(DeviceCtx* ctx, int slot) { return ctx->h_pick.as<uint8_t>() + 64 + 8 * slot; }
inline double* h_moments_at(DeviceCtx* ctx, int slot) { return ctx->h_moments.as<double>() + (size_t)slot * kFusedMomentDoubles; }

// ---- m3d_fit.cpp (stream_wait_spin: m3d_host_util.hpp)
int word_wait_spin(DeviceCtx* ctx, const uint32_t* word /* page-locked */, uint32_t seq);
int validate_fit_args(int kind, size_t n, bool has_normals, double prob);
uint64_t resolve_seed(const uint64_t* seed);
int finalize_deferred_refine(DeviceCtx* ctx, SegmentRounds& rounds);
int agree_seed(m3d_comm* comm, const uint64_t* seed, hipStream_t st, uint64_t* out);
int cloud_fit_locked(m3d_cloud* c, int kind, double thr, size_t max_iter, double prob, uint64_t seed, double* params,
                     size_t* inliers, size_t* n_inliers, m3d_stats* stats, FitCaller* caller = nullptr, m3d_comm* comm = nullptr);

// ---- m3d_refine.cpp
int compact_scratch(DeviceCtx* ctx, uint32_t nb, uint32_t** slots);
int exact_error(DeviceCtx* ctx, const CloudView& v, int kind, double thr,
                       const double* model_dev, uint64_t* count, double* error);
int approx_error_pair(DeviceCtx* ctx, const CloudView& v, int kind, double thr, const double* model_a,
                             const double* model_b, uint64_t* count_a, double* error_a, uint64_t* count_b, double* error_b);
int approx_error(DeviceCtx* ctx, const CloudView& v, int kind, double thr,
                        const double* model_dev, uint64_t* count, double* error);
int issue_refine_compaction(DeviceCtx* ctx, const CloudView& flag_view, const uint32_t* orig_dev, int kind, double thr,
                            const double* model_dev, const double* lazy_in, void* total_host, const FitCaller* caller,
                            Compaction* out, bool fused = false, uint64_t* idx_host = nullptr, const PartitionOut* part = nullptr,
                            bool allow_mask = true /* the list may come as a bit mask that refine() expands (m3d_config.list_mask) */);
int refine(DeviceCtx* ctx, const CloudView& flag_view, const CloudView& gather_view, const uint32_t* orig_dev, int kind, double thr,
           const double* model_dev, double* params_host /* in: best minimal model, out: refined */, size_t* inliers,
           size_t* n_inliers, int* general_fit_ok, int64_t expected_ni, const Compaction& queued /* on model_dev; empty: none */,
           const FitCaller* caller, bool hook_due = true /* false: caller->before_refine_wait has run already */,
           const double* lazy_in = nullptr /* pinned: the "in" value of params_host arrives with the wait */,
           bool fused = false /* model_dev is a minimal_fit_k record: moments ride on the compaction (needs lazy_in) */);

// ---- m3d_segmentation.cpp (the removal of a fit's inliers stays inside it)
int segment_impl(const double* xyz, size_t n, double threshold, int max_iteration, double min_ratio,
                        const uint64_t* seed, int device, m3d_comm* comm, size_t max_clusters, double* planes,
                        size_t* cluster_offsets, size_t* cluster_indices, size_t* n_clusters,
                        double* cluster_points = nullptr /* n x 3: the xyz of cluster_indices[i] at 3 i (may be null) */);
extern thread_local double g_seg_ms[6];   // the calling thread's last segmentation call (m3d_bench_last_segment_ms)

}  // namespace m3d
