// m3d_chunk_plan.hpp -- what a chunk of hypotheses will do, decided once (issue_chunk, m3d_fit.cpp).
//
//   ChunkRequest   what the caller asks for, by name
//   ChunkFacts     what the decisions read from the world (cloud, lane, slot, communicator, m3d_config), as plain values
//   ChunkPlan      every decision of the chunk and the sizes that go with them: plan_chunk(facts, request)
//
// issue_chunk's stages reserve and launch what the plan says and add only what a launch helper decides at run time (its return
// value).  No HIP here, no side effects: tests/cpp/test_chunk_plan.cpp compiles this header with plain g++ and holds every
// decision to its table.
#pragma once
#include "../../include/misc3d_amd.h"   // M3D_PLANE / M3D_SPHERE / M3D_CYLINDER

#include <algorithm>
#include <cstddef>
#include <cstdint>

struct m3d_comm;

namespace m3d {

struct PickFinal;
struct SegmentRounds;

constexpr uint32_t kPlanScoreTile = 2048;     // = kScoreTile (m3d_kernels.hpp), points per row of the dense scoring's partial counts
constexpr uint32_t kPlanPairReplicas = 1024;  // = kPairReplicas (m3d_cull_kernels.hpp); m3d_fit.cpp asserts both

struct ChunkRequest {
    size_t begin = 0, end = 0;   // the window of the hypothesis stream
    bool prune = false;          // fits only: hypotheses that cannot reach the best count of EARLIER ones are masked out
    uint32_t lead = 0;           // a fit's first chunk: the first `lead` hypotheses are counted on their own, for the incumbent
    bool new_fit = false;        // clears the running best count
    bool device_records = false;   // culled path: keep a device copy of the records in the slot's counts
    m3d_comm* comm = nullptr;    // hypotheses sharded over its ranks
    bool caller_ships_records = false;   // the caller queues pick_best_k behind the chunk and records the slot's `done` behind THAT
                                         // (an event between two kernels costs a ~5 us gap on this stream; behind pick_best_k
                                         // nothing follows at once)
    const PickFinal* pick_final = nullptr;   // one GPU: the chunk's last kernel takes pick_best_k's decision and stores the
                                             // completion word the host polls (no event)
    bool nothing_to_prune = false;   // the fit's ONLY chunk, issued without a lead pass: no incumbent will ever exist while it runs
    bool pre_wanted = false;     // a later chunk of a fit: MinimalFit and the box tests may go to the lane's pre-stream and run
                                 // under the scoring launches of the chunk before (the main stream waits for the slot's pre_done
                                 // in front of the keep masks) -- whether they do is the plan's decision (ChunkPlan::head)
    const double* move_best_from = nullptr;   // the fit's best minimal model lives in THIS slot's params, which the chunk is about
                                              // to overwrite: moved to the lane's best_params first, on the stream MinimalFit
                                              // will run on
    bool first_of_stream = false;   // m3d_cloud_score_shard, one rank, from hypothesis 0: a fit's first chunk in all but the
                                    // incumbent's clearing (the caller's): reference histograms as for new_fit
    SegmentRounds* rounds = nullptr;   // a segmentation's fit: the previous round's tombstone pass may be waiting to ride in this
                                       // chunk's minimal_fit_k launch
    double* ms_sample = nullptr;   // += host time spent filling the sample table
};

struct ChunkFacts {
    int kind = M3D_PLANE;
    uint32_t n_pad = 0;          // CloudView::n_pad
    uint32_t n_tiles = 0;        // SortedView::n_tiles
    double radius = __builtin_inf();   // SortedView::radius (inf: unknown, the fp64 box tests are used)
    bool has_dead = false;       // SortedView::has_dead
    bool has_frames = false;     // SortedView::frames exist
    bool has_pre_stream = false, has_pre_done = false;   // the lane's pre-stream, the slot's pre_done event
    bool tombstones_pending = false;   // ChunkRequest::rounds holds a tombstone pass that waits for a minimal_fit_k launch
    bool has_comm = false;       // ChunkRequest::comm, and of it:
    uint32_t world = 1, rank = 0;
    bool rccl = false;           // its transport is RCCL (a caller-supplied all-gather is always called)
    bool dense = false;          // m3d_config.dense_scoring or the calling thread's dense fit
    int cull_fp32 = 1, plane_bound = 1, ref_bound = 1, kernel_timing = 0;   // m3d_config
    int score_phases = 0;        // score_phases_for(kind)
};

enum class HeadStream { kMain, kPre };

struct ChunkPlan {
    // ---- sizes
    int m = 3;                   // sample indices per hypothesis
    uint32_t count = 0;          // hypotheses of the window
    uint32_t sl_pad = 0;         // hypotheses per rank, padded (one GPU: of the window)
    uint32_t h_pad = 0;          // padded length of the window's arrays: sl_pad x world
    uint32_t n_groups = 0;       // h_pad / 64
    uint32_t g0 = 0, g1 = 0;     // this rank's groups [g0, g1) of the chunk
    uint32_t ga = 0;             // groups of the lead pass (0: none)
    uint32_t g_lo = 0;           // first group of this rank's behind the lead: the window of the main scoring is [g_lo, g1)
    uint32_t dense_tiles = 0;    // rows of the dense path's partial counts
    // ---- the head: sample table, minimal_fit_k, box tests
    HeadStream head = HeadStream::kMain;
    bool tombstones_ride = false;   // the pending tombstone pass is offered to the minimal_fit_k launch
    bool dense = false;
    bool cull32 = false;         // fp32 box tests: minimal_fit_k writes their records
    bool prune_scratch = false;  // touched-tile counters, phase counters, bound sums: the slot's ub
    bool lead_prepared = false;  // minimal_fit_k sets up the lead pass (keep masks, counter replicas) itself
    bool all_prepared = false;   // ... or ALL groups: no keep_mask_k launch at all
    // ---- the culled path
    bool own_real = false;       // this rank's slice holds real hypotheses (a short last window can leave the highest ranks without)
    bool prune = false;
    bool fuse_lead = false;      // try cull_lead_k: the chunk's box tests and its lead pass in one launch
    bool lead_elsewhere = false; // rank > 0: the lead is somebody else's slice, its box tests a launch of their own
    bool phased = false;         // phased scoring is eligible (launch_score_phased still decides)
    bool bound_on = false, bound_forced = false;   // the histogram bound runs; ... whatever the length of its list
    bool ref_on = false;         // ... with the reference-plane histograms
    uint32_t ref_min_count = 0;  // ... RefHistArgs::min_count: the lead's best count below which no histograms are built
    bool touched_wanted = false; // cylinders: the box tests also write a word per hypothesis and 64 tiles -- unless cull_lead_k ran
    uint32_t ubsum_at = 0;       // ... where its sums start inside the slot's ub, in words
    bool timing = false;         // events around the scoring launches
    // ---- the records
    bool solo = false;           // a communicator of ONE rank over RCCL: the gather is the identity
    bool records_to_host = false;   // the folding kernels write the records into the slot's pinned array themselves
    bool records_on_device = false; // ... and / or into the slot's counts
    bool counts_reserved = false;   // the slot's counts are needed at all
    bool polls = false;          // completion is the PickFinal's word, not the `done` event
};

// Where the planes' histogram bound is worth its launch: plane_bound_k costs 12-25 us per window whatever it prunes, and it halves
// a scoring launch -- worth it when that launch is long.  Measured on C2-shaped clouds, resident, ms per fit without / with:
//   points x hypotheses   50 k x 3000 0.103 / 0.135   150 k x 10 000 0.166 / 0.178   150 k x 40 000 0.325 / 0.377   400 k x 10 000 0.176 / 0.175
//   400 k x 40 000 0.413 / 0.386   1 M x 3000 0.207 / 0.213   1 M x 10 000 0.300 / 0.274   1 M x 40 000 0.654 / 0.606
//   4 M x 3000 0.530 / 0.569   4 M x 10 000 0.864 / 0.809   4 M x 40 000 1.876 / 1.671
// i.e. windows of 8192 hypotheses and more on tiles x hypotheses >= 1.5e7.
inline bool bound_pays(uint32_t n_tiles, size_t window_hypotheses) {
    return window_hypotheses >= 8192 && (double)n_tiles * (double)window_hypotheses >= 1.5e7;
}

// m3d_config.plane_bound as a fit of `kind` sees it: forcing the reference histograms (ref_bound = 2, the tests' switch) forces the
// launch they live in
inline int bound_mode(int kind, int plane_bound, int ref_bound) {
    return (plane_bound != 0 && kind == M3D_PLANE && ref_bound == 2) ? 2 : plane_bound;
}

// Can the head of ANY chunk of a fit leave the main stream?  The part of plan_chunk's decision that holds for a whole fit: what
// its caller asks before it records the pre-stream's gate in front of the first chunk.
inline bool pre_stream_possible(bool dense, bool has_comm) { return !dense && !has_comm; }

// The fp32 box tests (cull_tiles32_k) replace the fp64 ones when the cloud's extent is known
inline bool box_tests_fp32(const ChunkFacts& f) { return !f.dense && f.cull_fp32 != 0 && f.radius < 1e18; }

inline ChunkPlan plan_chunk(const ChunkFacts& f, const ChunkRequest& r) {
    ChunkPlan p;
    const bool comm = f.has_comm;
    const uint32_t world = comm ? f.world : 1u, rank = comm ? f.rank : 0u;
    const auto round_up64 = [](uint32_t v) { return (v + 63u) / 64u * 64u; };
    p.m = f.kind == M3D_PLANE ? 3 : (f.kind == M3D_SPHERE ? 4 : 2);
    p.count = (uint32_t)(r.end - r.begin);
    p.dense = f.dense;
    p.prune = r.prune;
    p.timing = f.kernel_timing != 0;
    p.tombstones_ride = f.tombstones_pending && f.kind == M3D_PLANE;
    // where the chunk's head runs -- decided ONCE, here, in front of everything that depends on it (the record
    // move used to repeat a part of this condition in the caller)
    const bool pre = r.pre_wanted && pre_stream_possible(f.dense, comm) && r.prune && !r.new_fit && r.lead == 0 &&
                     !f.tombstones_pending && f.has_pre_stream && f.has_pre_done;
    p.head = pre ? HeadStream::kPre : HeadStream::kMain;
    // Sharded fits: the chunk is the SAME window on every rank, the box tests and the scoring cover this rank's slice of sl_pad
    p.sl_pad = round_up64((p.count + world - 1) / world);
    p.h_pad = comm ? p.sl_pad * world : round_up64(p.count);
    p.n_groups = p.h_pad / 64;
    p.dense_tiles = f.n_pad / kPlanScoreTile;
    p.g0 = comm ? rank * (p.sl_pad / 64) : 0u;
    p.g1 = comm ? p.g0 + p.sl_pad / 64 : p.n_groups;
    p.own_real = (size_t)p.g0 * 64 < p.count;
    p.cull32 = box_tests_fp32(f);
    p.prune_scratch = !f.dense && r.prune;
    // the records: a sharded fit gathers them on the device; the dense path copies them from there
    p.records_on_device = !f.dense && (r.device_records || comm);
    p.counts_reserved = f.dense || r.device_records || comm;   // (culled path otherwise: the records go straight to h_counts)
    // sharded: the host gets the GATHERED records -- unless the communicator has ONE rank: its slice is the window, the
    // gather the identity, and the records go to the host the way the one-GPU path sends them (written by the folding
    // kernels themselves: no copy command, no detour over the copy stream)
    p.solo = comm && f.world == 1 && f.rccl;
    p.records_to_host = !f.dense && (!comm || p.solo);
    p.polls = r.pick_final != nullptr && !f.dense && p.own_real;
    // lead > 0 (a fit's first chunk): the first `lead` hypotheses are counted on their own, and their best
    // count then prunes the rest of the SAME chunk -- what a separate small first chunk did, without its
    // own sample copy, MinimalFit and box-test launches.  The records are complete after the second pass.
    // (decided in front of minimal_fit_k, which prepares the lead pass of a NEW fit itself: see LeadPrep)
    const bool use_lead = !f.dense && r.prune && r.lead >= 64 && r.lead % 64 == 0 && r.lead + 64 <= p.count &&
                          (!comm || p.sl_pad >= r.lead + 64);
    p.ga = use_lead ? r.lead / 64 : 0u;
    p.g_lo = std::max(p.g0, p.ga);
    p.lead_prepared = use_lead && r.new_fit && p.own_real && r.lead <= p.h_pad && kPlanPairReplicas <= p.h_pad;
    // no lead pass and nothing to prune against (a new fit's only chunk on one GPU, FitCaller::no_prune_hint): the same
    // set-up for ALL groups -- keep everything, clear every counter replica -- and no keep_mask_k launch
    p.all_prepared = r.nothing_to_prune && !use_lead && r.lead == 0 && !f.dense && r.prune && r.new_fit && !comm &&
                     kPlanPairReplicas <= p.h_pad;
    if (f.dense || !p.own_real) return p;

    // fp32 box tests and fp32 screen on: the box tests of the chunk (this rank's slice) and the counting of its leading groups
    // share ONE launch (cull_lead_k; the lead pass runs its own box tests) -- two latency-bound launches less the
    // time of one.  (sharded fits: the rank that owns the leading groups)
    p.fuse_lead = p.ga && p.g0 == 0 && p.cull32;
    p.lead_elsewhere = p.ga && p.g0 >= p.ga;
    // an incumbent exists: this chunk's lead pass, or earlier chunks / windows -- sharded fits included: every rank prunes its
    // slice against the same incumbent
    const bool incumbent = use_lead || !r.new_fit;
    // phased scoring (launch_score_phased): an incumbent exists, the fp32 box tests run (they count the touched tiles per
    // phase), no tombstones
    p.phased = r.prune && incumbent && p.cull32 && !f.has_dead && f.score_phases != 0;
    // planes with an incumbent and tile frames: a histogram upper bound per touched (tile, hypothesis) pair replaces
    // "512 per touched tile" in the keep rule (m3d_bound.hip).  The keep kernels hand plane_bound_k the kept
    // hypotheses as a list (its length: word 6 of best_count); the sums go to the slot's phase-counter array, zeroed by
    // minimal_fit_k and unused when the scoring is not phased.
    // Spheres and cylinders (round 5): the same bound with the shell taken as a slab per tile (cyl_pair_ub); cylinders in front of
    // the phased scoring -- whose phase counters sit where the bound sums go otherwise, so theirs get the block behind them.
    // (Spheres: C3's fit loses a third of its (tile, hypothesis) pairs and gains nothing -- 0.77 ms with and without, the bound's
    // launch costs what it saves; theirs runs when the bound is forced, m3d_config.plane_bound = 2, i.e. in the tests.)
    const int mode = bound_mode(f.kind, f.plane_bound, f.ref_bound);
    p.bound_forced = mode == 2;
    p.bound_on = (f.kind == M3D_CYLINDER || !p.phased) && r.prune && f.has_frames && mode != 0 &&
                 (mode == 2 || (f.kind != M3D_SPHERE && bound_pays(f.n_tiles, comm ? p.sl_pad : p.count))) && incumbent &&
                 p.g_lo < p.g1;
    if (p.bound_on) p.ubsum_at = p.phased ? 2 * p.h_pad : p.h_pad;
    // planes, the first chunk of a one-GPU fit with a lead pass, no tombstones: a second histogram per tile, along the lead's
    // best plane (m3d_ref_hist.hpp) -- written by extra workgroups of the lead_fold_keep_k launch, read by plane_bound_k
    p.ref_on = p.bound_on && f.kind == M3D_PLANE && !p.phased && !comm && (r.new_fit || r.first_of_stream) && p.ga && p.g0 == 0 &&
               !f.has_dead && f.ref_bound != 0 && (f.ref_bound == 2 || bound_pays(f.n_tiles, p.count));
    // uniform clutter gains nothing and must not pay for the pass: no histograms unless the lead's best plane holds 8
    // points per tile, 1 / 64 of the cloud (1 M x 10 000 clutter: the best plane holds 1 / 141; measured in
    // profiles/r09_ref_bound.txt); forced: any count
    if (p.ref_on) p.ref_min_count = f.ref_bound == 2 ? 1u : 8u * f.n_tiles;
    // cylinders in front of the bound: the box tests also leave a word per hypothesis and 64 tiles (cull_hyp32_k), which
    // plane_bound_k reads instead of repeating the tests
    p.touched_wanted = p.bound_on && f.kind == M3D_CYLINDER && p.cull32 && !p.lead_elsewhere && p.g1 - p.g0 >= 128u;
    return p;
}

}  // namespace m3d
