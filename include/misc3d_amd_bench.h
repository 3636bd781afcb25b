/*
 * misc3d_amd_bench.h -- measurement hooks of libmisc3d_amd.so.  NOT part of the drop-in boundary: nothing here
 * replaces a function of the reference; bench.py / tools/ use it to time single kernels for the `roofline`
 * objects.  Kept apart from include/misc3d_amd.h so that the product header holds only what a reference caller binds.
 */
#ifndef MISC3D_AMD_BENCH_H
#define MISC3D_AMD_BENCH_H

#include "misc3d_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* average duration in ms of the scoring kernel alone
 * (score_k, the dominant kernel) over `reps` launches of `n_hypotheses` hypotheses, timed with HIP
 * events on the library's own stream after one untimed launch.  Not part of the reference. */
int m3d_bench_time_score(m3d_cloud *cloud, int kind, double threshold, const uint32_t *samples,
                         size_t n_hypotheses, int reps, int mode, double *ms_avg,
                         uint64_t *listed_pairs);
/* mode 0: score_list_k (production: counting over the (tile, hypothesis) pairs that survive the box
 * test); mode 1: cull_k (the box tests); mode 2: score_k (dense: every tile x every hypothesis).
 * listed_pairs (may be NULL): number of surviving (tile, hypothesis) pairs, tile = 512 points. */


/* fp64 VALU issue rate the device sustains (independent v_mul_f64 / v_add_f64 chains, no FMA, no memory traffic) over
 * about `ms_target` milliseconds of that load, in 1e12 lane-operations per second: the attainable counterpart of the
 * nominal 39.3 (256 CU x 4 SIMD x 16 lanes x 2.4 GHz) -- the chip clocks below 2.4 GHz under sustained fp64 load. */
int m3d_bench_fp64_issue_rate(int device, double ms_target, double *tera_lane_ops_per_s, double *ms_measured);

/* m3d_cloud_create's own wall clock in ms: out[0] = the whole call (always); with m3d_config.kernel_timing set when the
 * cloud was created also the phases, each closed by a stream synchronisation: out[1] = host-to-device copies of the
 * caller's arrays + AoS -> SoA transposes, out[2] = bounding box of the device copy incl. its round trip, out[3] =
 * Hilbert counting sort, out[4] = tile boxes + the tiles' fp32 offsets ("report upload separately"). */
int m3d_bench_cloud_setup_ms(const m3d_cloud *cloud, double out[5]);

/* 1 when [p, p + bytes) lies inside a live block of m3d_host_alloc (the registry the fits consult before the device writes, or
 * the host expands a mask, straight into a caller's array), else 0.  What tests/test_gpu_host_blocks.py holds the two kinds of
 * block to: reported inside their bounds, not past them, not after m3d_host_free. */
int m3d_bench_host_block(const void *p, size_t bytes);

/* plane_bound_k (m3d_bound.hip) on its own: ub_out[h] = the histogram upper bound of hypothesis h's inlier count, for EVERY
 * hypothesis of the sample table (n_hypotheses x 3 indices, at most 16 384; nothing is pruned).  What
 * tests/test_gpu_plane_bound.py holds against the exact counts of m3d_cloud_score_range: ub >= count, hypothesis by hypothesis.
 * Builds the cloud's tile frames if it has none yet. */
int m3d_bench_plane_upper_bounds(m3d_cloud *cloud, double threshold, const uint32_t *samples, size_t n_hypotheses,
                                 uint32_t *ub_out);
/* ... from the reference-plane histograms alone (ref_hist_tile / ref_pair_ub): the reference is hypothesis ref_index of the table;
 * a pair the reference bound does not cover (a hypothesis more than acos 0.9 off the reference) counts 512.  What
 * tests/test_gpu_ref_bound.py holds against the exact counts. */
int m3d_bench_plane_ref_upper_bounds(m3d_cloud *cloud, double threshold, const uint32_t *samples, size_t n_hypotheses,
                                     size_t ref_index, uint32_t *ub_out);
/* ... for any kind (M3D_PLANE / M3D_SPHERE / M3D_CYLINDER; samples: n_hypotheses x 3 / 4 / 2 indices): spheres and cylinders are
 * bounded through the slab their shell is over one tile (m3d_bound_fp.hpp cyl_pair_ub). */
int m3d_bench_upper_bounds(m3d_cloud *cloud, int kind, double threshold, const uint32_t *samples, size_t n_hypotheses,
                           uint32_t *ub_out);
/* Wall clock of the calling thread's LAST m3d_segment_plane_iterative* call in ms: out[0] the whole call, out[1]
 * m3d_cloud_create (upload, sort, tile boxes), out[2] the round loop, out[3] the final copy of the index lists out of
 * the page-locked staging array (0 when the caller's array is page-locked), out[4] of the round loop: the rounds on more
 * than an eighth of the cloud, out[5] = their number + 1e-4 x all rounds. */
int m3d_bench_last_segment_ms(double out[6]);

/* TEST hook (tests/fp_order_worker.py): the EdgeLength + Distance checkers of the registration path evaluated on the
 * HOST by the very code the kernels compile (m3d_reg_fp.hpp reg_checkers): ps / pd = the 3 sampled source / target
 * points (3 x 3 doubles each), T = 4 x 4 row-major.  Returns 1 = pass, 0 = rejected.  Lets a box without a GPU check
 * that a library built for another M3D_FP_ORDER carries that association into the registration code as well. */
int m3d_bench_reg_checkers(const double *ps, const double *pd, const double *T, double edge_threshold,
                           double distance_threshold);

/* TEST hook (tests/test_gpu_reg_sums.py): the 18 sums m3d_kabsch reads back for n point pairs (n x 3 row-major doubles each),
 * from the upload, launch and read-back m3d_kabsch itself makes -- out[0..2] / [3..5] = the coordinate sums of src / dst,
 * out[6 + 3 r + c] = sum (dst_r - mean dst_r)(src_c - mean src_c), out[15..17] = sum (src_k - mean src_k)^2, the means being the
 * kernels' own (coordinate sum * (1 / n)).  Arguments are checked as m3d_kabsch checks them (n >= 3). */
int m3d_bench_kabsch_sums(const double *src, const double *dst, size_t n, int device, double out[18]);

/* TEST hook (tests/test_gpu_reg_sums.py): ONE evaluation of the point-to-point ICP step under the pose T (4 x 4 row-major), by
 * the launches m3d_registration_icp and m3d_information_matrix make on the target grid m3d_registration_icp builds: the source
 * moved by T, its nearest target points within max_correspondence_distance, then out[0] = the sum of their squared distances,
 * out[1] = their number, out[2..19] = the 18 sums of the next update over the correspondence set (laid out as in
 * m3d_bench_kabsch_sums, means = coordinate sum * (1 / out[1])), out[20..28] = the moments of the matched target points
 * (x y z xx yy zz xy xz yz); corr (may be NULL): n_src entries, the target index of source point i or -1.  An empty cloud:
 * all zeros, every corr -1. */
int m3d_bench_icp_sums(const double *src, size_t n_src, const double *dst, size_t n_dst, double max_correspondence_distance,
                       const double *T, int device, double out[29], int64_t *corr);

/* MEASUREMENT / TEST hook (tools/bench_configs.py P1 / P2, tests/test_gpu_fps.py): the device path of every later
 * m3d_farthest_point_sampling in the process -- 0 = by size (the default), M3D_FPS_PATH_SINGLE (n <= 8192),
 * M3D_FPS_PATH_PRUNED, M3D_FPS_PATH_DENSE (the pruned path's steps with no tile skipped: the A/B reference).  The
 * result does not depend on it. */
int m3d_bench_fps_force_path(int path);

/* MEASUREMENT / TEST hook (tools/bench_configs.py K3, tests/test_gpu_knn.py): the device path of every later m3d_knn_search
 * in the process -- 0 = by shape (the default), M3D_KNN_PATH_GRID, M3D_KNN_PATH_TILE, M3D_KNN_PATH_SELECT.  A forced
 * path applies wherever it can: GRID only for dim 3 and kout <= 128 (else by shape), TILE for kout <= 128 (else
 * SELECT), SELECT always (in pages of 16 rather than 128, so that small kout run several pages).  The result does not
 * depend on it. */
int m3d_bench_knn_force_path(int path);

/* TEST hook (tests/test_gpu_knn_seams.py): launch_knn_tile + launch_knn_merge as run_tile issues them, for ONE chunk of m
 * queries, `pages` pages of kk pairs (page p > 0 above the floor page p - 1 left), over `splits` splits of rows_per_split rows.
 * idx_out / d2_out: m x (pages kk), raw -- a slot no row fills holds the kernels' sentinel (index 0xFFFFFFFF, key all ones).
 * M3D_ERR_INVALID_ARG unless 1 <= kk <= 128, pages >= 1, 1 <= splits <= 256, rows_per_split >= 1, splits x rows_per_split >= n
 * (trailing empty splits are allowed: a list of sentinels), 1 <= dim <= 1024, m >= 1, n >= 1 and the chunk's scratch
 * (m3d_knn_search's own bound, 256 MiB) holds. */
int m3d_bench_knn_tile_merge(const double *data, size_t n, int dim, const double *queries, size_t m, int kk, int pages,
                             int splits, uint32_t rows_per_split, int device, uint32_t *idx_out, uint64_t *d2_bits_out);

/* MEASUREMENT / TEST hook (tests/test_gpu_voxel.py): the key path of every later m3d_voxel_down_sample* in the process --
 * 0 = by the key widths (the default), M3D_VOXEL_PATH_PACKED (where the keys fit 63 bits, else wide), M3D_VOXEL_PATH_WIDE.
 * The result does not depend on it. */
int m3d_bench_voxel_force_path(int path);

/* TEST hook (tests/test_proximity.py): the cut-offs m3d_proximity_segment derives on the host for an evaluator
 * (m3d_proximity_fp.hpp) -- out[0] = d2_cut (Distance: dist < t <=> d2 < d2_cut; DistanceNormals: dist >= t <=>
 * d2 >= d2_cut), out[1..4] = lo1, hi1, lo2, hi2 (the angle test accepts dot exactly on [lo1, hi1] u [lo2, hi2]). */
int m3d_bench_proximity_cutoffs(double dist, double angle_deg, double out[5]);

/* TEST hook (tests/test_grid_ladder.py, tests/test_gpu_grid_ladder.py): the rung of the cell-table ladder a radius grid lands on
 * (radius_grid_geom, m3d_grid_geom.hpp) for the box [lo, hi], searches within `edge` (> 0) and K0 (1..16) cells per edge --
 * K = the cells per edge that fitted, h = the cell edge, dims = the cells per axis, pads included.  The tests assert through it
 * that each of their scenes sits on the rung it is meant for. */
int m3d_bench_radius_grid_geom(const double lo[3], const double hi[3], double edge, int K0, int *K, double *h, uint64_t dims[3]);
/* ... and the K0 the registration validation starts that ladder from for m3d_config.reg_cells_per_radius = k_cfg and a target
 * of n_dst points (reg_grid_k0). */
int m3d_bench_reg_grid_k0(int k_cfg, uint64_t n_dst);

/* TEST hook (tests/test_fpfh.py): the FPFH pair features and the bin rule evaluated on the HOST by the very code the
 * kernels compile (m3d_fpfh_fp.hpp) -- pairs: m x 12 doubles (p1, n1, p2, n2), bins: m x 3 (columns of the 33-row),
 * features (may be NULL): m x 3 (f0, f1, f2). */
int m3d_bench_fpfh_pair_bins(const double *pairs, size_t m, int32_t *bins, double *features);

/* TEST hook (tests/test_gpu_fpfh_stages.py): m3d_compute_fpfh's own job -- the same kernels in the same order on one grid, the
 * normals given -- with its stages taken out after the call's last synchronisation, all by POINT index (not query order); every
 * output may be NULL.  list_idx (n x max_nn), list_d2 (n x max_nn), cnt (n): the neighbour lists and the Hybrid counts as
 * fpfh_spfh_k and fpfh_fpfh_k read them, that is entries [0, cnt); an entry at or past cnt is 0xFFFFFFFF / +inf, a non-finite
 * point has cnt 0.  spfh_count (n x 33), spfh_incr (n): the SpfhRows as fpfh_fpfh_k reads them (after the host-decided rows
 * were scattered); zeros for a non-finite point, whose row the device never writes.  tie_points (capacity n), *n_ties: the
 * points fpfh_spfh_k listed for the host, ascending.  feature_out (n x 33): the call's result.  Arguments are checked as
 * m3d_compute_fpfh checks them. */
int m3d_bench_fpfh_stages(const double *xyz, const double *normals, size_t n, int search, double radius, int max_nn, int device,
                          uint32_t *list_idx, double *list_d2, uint32_t *cnt, uint8_t *spfh_count, double *spfh_incr,
                          uint32_t *tie_points, uint64_t *n_ties, double *feature_out, m3d_fpfh_stats *stats);

/* TEST hook (tests/test_gpu_match_sliced.py): which way the CALLING THREAD's last m3d_match_mutual_nn went -- bit 0: the split-fp16
 * MFMA screen produced the result, bit 1: the matrices went up in slices under the scan (m3d_config.match_pipeline), bit 2: a
 * later slice did not fit the scale chosen from the first ones and the search was redone whole on the resident matrices,
 * bit 3: the fp32 screen, bit 4: fp64 brute force. */
unsigned m3d_bench_match_last_path(void);

/* MEASUREMENT / TEST hook (tools/bench_configs.py, tests/test_gpu_ppf.py): every later m3d_ppf_vote in the process keeps its
 * accumulators in device memory when device_memory_path != 0 (0: by (n, alpha_model_num), the default), and runs at most
 * max_groups workgroups (0: as many as the scratch allows, the default; a small value makes each workgroup take several
 * reference positions in turn).  The result does not depend on either. */
int m3d_bench_ppf_force(int device_memory_path, int max_groups);

/* MEASUREMENT / TEST hook (tests/test_gpu_ppf_cluster.py): every later m3d_ppf_cluster_poses / m3d_ppf_estimate in the
 * process lets `splits` workgroups share the j tiles of a row block of the pair kernels (0: by the number of row blocks, the
 * default).  The result does not depend on it. */
int m3d_bench_ppf_cluster_force(int splits);

/* TEST hook (tests/test_gpu_scratch_fill.py): what a block of device or page-locked scratch holds when the library hands it
 * out -- pattern -1 = whatever it held (the default: a fresh allocation, or a block of the lane's free list with the last
 * call's contents), 0..255 = every byte of the block set to `pattern` before it is handed out, fresh or recycled.  A buffer
 * that is large enough already is not handed out again and keeps its contents.  Filling waits for the whole device on both
 * sides of the write.  Switching resets the counters of m3d_bench_scratch_fill_stats.  No result depends on it. */
int m3d_bench_scratch_fill(int pattern);
/* ... out[0] = the blocks, out[1] = the bytes filled since the last m3d_bench_scratch_fill. */
int m3d_bench_scratch_fill_stats(uint64_t out[2]);
/* ... takes a lane of `device` as a one-call entry point does, takes one block of device scratch of `bytes` (>= 64) bytes,
 * copies the block's first 64 bytes to first_last[0..63] and its last 64 to first_last[64..127], and gives the block back. */
int m3d_bench_scratch_probe(int device, size_t bytes, unsigned char first_last[128]);

#ifdef __cplusplus
}
#endif
#endif /* MISC3D_AMD_BENCH_H */
