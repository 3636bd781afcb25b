/*
 * misc3d_amd.h -- C ABI of the MI355X (gfx950) implementation of the Misc3D RANSAC hot path.
 *
 * This is the drop-in boundary: every entry point replaces one function of the reference
 * (yuecideng/Misc3D; paths below are relative to its repository root).  Plain pointers and sizes,
 * no C++/torch types.  Inputs are borrowed for the duration of the call; outputs go to
 * caller-allocated buffers; nothing allocated inside crosses the ABI except opaque handles that
 * are released with the matching *_destroy.
 *
 * Return convention (mirrors the reference's three outcomes):
 *     1  reference returned `true`
 *     0  reference returned `false` (soft failure: params are zeroed by the callers exactly as
 *        python/py_common.cpp:21-23,39-41,61-63 do; inliers are still returned)
 *    <0  the reference raises (misc3d::LogError throws std::runtime_error, src/logging.cpp:64-74):
 *        M3D_ERR_* below; m3d_last_error() gives the reference's message text.
 * The library never throws and never falls back to a CPU path: without a usable HIP device every
 * compute entry point returns M3D_ERR_DEVICE.
 *
 * Point clouds are Open3D's layout: contiguous N x 3 float64 (open3d::geometry::PointCloud::points_
 * is std::vector<Eigen::Vector3d>, 24-byte POD elements), so `pcd.points_.data()->data()` can be
 * passed as is.
 */
#ifndef MISC3D_AMD_H
#define MISC3D_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M3D_OK 1
#define M3D_FALSE 0
#define M3D_ERR_PROBABILITY (-1) /* "Probability must be > 0 or <= 1.0"          ransac.h:483-485 */
#define M3D_ERR_TOO_FEW_POINTS (-2) /* "Can not fit model due to lack of points" ransac.h:510-513;
                                       "The number of points pair is less than 3." transform_estimation.cpp:17-19,130-133 */
#define M3D_ERR_NO_NORMALS (-3) /* "Fit cylinder requires normals."            py_common.cpp:50-52, ransac.h:356-359 */
#define M3D_ERR_SIZE_MISMATCH (-4) /* "The number of points pair is not equal." transform_estimation.cpp:20-22 */
#define M3D_ERR_INVALID_ARG (-5) /* null pointer / out-of-range index / N >= 2^31 */
#define M3D_ERR_DEVICE (-6) /* no HIP device, HIP runtime error, or out of device memory */
#define M3D_ERR_INTERNAL (-7) /* self-check failed (counts from the scoring kernel and the refine pass disagree) */
#define M3D_ERR_NON_FINITE (-8) /* m3d_voxel_down_sample: a point with a non-finite coordinate (the reference's int(floor(..)) is undefined);
                                   m3d_raycast_pinhole: a vertex that is not finite in single precision under its pose */

enum m3d_model_kind { M3D_PLANE = 0, M3D_SPHERE = 1, M3D_CYLINDER = 2 };

/* Observable state of misc3d::common::RANSAC after FitModel (ransac.h:616-619 logs fitness and
 * count) plus counters of this implementation. */
typedef struct m3d_stats {
    double fitness;              /* best inlier ratio (ransac.h:617) */
    double inlier_rmse;          /* best error/sqrt(n) if it had to be evaluated (ties), else NaN */
    uint64_t count;              /* valid hypotheses evaluated before the adaptive stop ("run {} iterations") */
    uint64_t iterations;         /* loop index at which the reference loop went idle */
    int64_t best_index;          /* hypothesis index of the best model, -1 if none */
    int32_t general_fit_ok;      /* RefineModel's return (ransac.h:548) */
    int32_t ties;                /* equal-fitness comparisons (ransac.h:596) decided during the replay */
    uint64_t hypotheses_scored;  /* hypotheses the GPU scored (>= iterations: speculative chunks) */
    uint64_t exact_rmse_evals;   /* serial-order error sums needed (ties that order-free sums could not decide) */
    double ms_sample;            /* host: std::mt19937 sample table */
    double ms_score;             /* host clock: sampling, minimal fit, scoring and replay, from the first launch to the last replayed chunk (filled with m3d_config.kernel_timing) */
    double ms_refine;            /* device+host: inlier compaction, GeneralFit, copy-out */
    double ms_total;             /* wall clock of the call */
    double ms_score_kernel;      /* device: sum of the scoring-kernel launches alone (HIP events around each; m3d_config.kernel_timing) */
    uint32_t score_launches;     /* number of scoring-kernel launches (chunks) behind ms_score_kernel */
    uint32_t early_pick_redone;  /* 1: RefineModel had been started on the device's own pick of the winner (probability-1
                                  * fits) and the sequential replay chose another hypothesis (rmse tie): it was run again */
    uint64_t pairs_scored;       /* (512-point tile, hypothesis) pairs those launches evaluated after culling and pruning */
    uint64_t pairs_exact;        /* ... of which the fp32 screen (m3d_config.score_fp32_screen) left to the exact fp64 code */
    uint64_t pairs_timed;        /* ... of pairs_scored: evaluated by the launches behind ms_score_kernel / score_launches.  Smaller than
                                    pairs_scored when the leading hypotheses of a fit's first chunk were counted inside cull_lead_k
                                    (one launch for the box tests and the lead pass: one GPU, fp32 paths on), which is not timed */
} m3d_stats;

/* ---- one-shot fits: python/py_common.cpp:11-67 FitPlane / FitSphere / FitCylinder ------------- */
/* seed: NULL = std::random_device (reference behaviour, utils.h:74-77); else std::mt19937(*seed).
 * device: HIP device ordinal.  inliers: capacity n.  params: 4 (plane a,b,c,d; sphere cx,cy,cz,r)
 * or 7 (cylinder px,py,pz,nx,ny,nz,r).  On return 0 the caller zeroes params (py_common.cpp:21-23). */
int m3d_fit_plane(const double *xyz, size_t n, double threshold, size_t max_iteration,
                  double probability, const uint64_t *seed, int device, double params[4],
                  size_t *inliers, size_t *n_inliers, m3d_stats *stats);
int m3d_fit_sphere(const double *xyz, size_t n, double threshold, size_t max_iteration,
                   double probability, const uint64_t *seed, int device, double params[4],
                   size_t *inliers, size_t *n_inliers, m3d_stats *stats);
int m3d_fit_cylinder(const double *xyz, const double *normals, size_t n, double threshold,
                     size_t max_iteration, double probability, const uint64_t *seed, int device,
                     double params[7], size_t *inliers, size_t *n_inliers, m3d_stats *stats);

/* ---- resident cloud: RANSAC::SetPointCloud (ransac.h:469-475) keeps a copy; here the copy lives
 *      in HBM as SoA x[],y[],z[] (+ normals) so repeated fits do not re-upload. ------------------ */
typedef struct m3d_cloud m3d_cloud;
m3d_cloud *m3d_cloud_create(const double *xyz, const double *normals /* may be NULL */, size_t n,
                            int device);
void m3d_cloud_destroy(m3d_cloud *cloud);
/* Device blocks released by the library (destroyed clouds, per-call scratch of the registration / matcher / normals /
 * boundary entry points) are parked on a per-device free list (at most m3d_config.pool_limit_mb, default 4 GiB) and handed out again instead of going
 * through hipFree / hipMalloc on every call; this returns them, and the upload scratch, to the driver. */
void m3d_release_cached(int device);
/* Page-locked host memory for OUTPUT buffers (inlier index lists).  Any host pointer is accepted wherever this
 * header takes an output buffer; one obtained here lets the library start the device-to-host copy of the index
 * list as soon as the list exists, overlapped with the GeneralFit sums, instead of last (a copy into pageable
 * memory occupies the calling thread until it is done).  NULL + m3d_last_error() on failure. */
void *m3d_host_alloc(size_t bytes);
void m3d_host_free(void *p);
/* Points currently in the cloud (shrinks with m3d_cloud_remove_inliers) / points it was created with. */
size_t m3d_cloud_size(const m3d_cloud *cloud);
size_t m3d_cloud_original_size(const m3d_cloud *cloud);
/* RANSAC::SetProbability + SetMaxIteration + FitModel (ransac.h:482-516) on the resident cloud.
 * inliers may be NULL (then only *n_inliers is reported). */
int m3d_cloud_fit(m3d_cloud *cloud, int kind, double threshold, size_t max_iteration,
                  double probability, const uint64_t *seed, double *params, size_t *inliers,
                  size_t *n_inliers, m3d_stats *stats);

/* ---- many short fits in ONE call (round 6).  The reference's fits are called one at a time from Python
 * (python/py_common.cpp:11-78 under its callers' loops); a resident fit of a few dozen hypotheses takes ~80 us on the device, and
 * threads of such calls are serialised by what the binding does per call under the interpreter's lock, not by the library's
 * lanes.  A batch hands the loop over: the jobs of one cloud run in the order given, clouds that live on different lanes of a
 * device (m3d_cloud_create_lane) or on different devices run side by side on threads of the library -- one call, one release of
 * the interpreter's lock.  Every job carries its own rc (m3d_cloud_fit's: 1 / 0 / < 0) and outputs; the call returns M3D_OK, or
 * the first failing job's error code with m3d_last_error() = "job <k>: ...".  inflight: lanes worked at a time (0 = all). */
typedef struct m3d_fit_job {
    m3d_cloud *cloud;
    int32_t kind, has_seed;
    double threshold, probability;
    uint64_t max_iteration, seed;
    size_t *inliers;           /* capacity: the cloud's size; may be NULL (then only n_inliers is reported) */
    double params[8];          /* out */
    uint64_t n_inliers;        /* out */
    int32_t rc, reserved_;     /* out */
    m3d_stats stats;           /* out */
} m3d_fit_job;
int m3d_cloud_fit_batch(m3d_fit_job *jobs, size_t n_jobs, int inflight);
/* m3d_cloud_create on a lane of the caller's choice (0 .. m3d_config.lanes - 1; < 0: the calling thread's own, as m3d_cloud_create):
 * a single-threaded caller that wants its clouds' fits to overlap (m3d_cloud_fit_batch) spreads them over the lanes itself. */
m3d_cloud *m3d_cloud_create_lane(const double *xyz, const double *normals /* may be NULL */, size_t n, int device, int lane);

/* ---- hypothesis-range scoring: the shardable unit (ransac.h:572-590 body for i in [begin,end)).
 * samples: H x m sample indices (m = 3 plane, 4 sphere, 2 cylinder) as the sequential sampler
 * (utils.h:81-97) produces them; m3d_draw_samples reproduces that table from a seed.
 * Outputs (host, length end-begin): valid = MinimalFit's return, counts = inlier_num of
 * EvaluateModel (ransac.h:626-641), models = (end-begin) x 8 doubles (first 4/7 = parameters).
 * Any of counts/valid/models may be NULL. */
int m3d_draw_samples(size_t n_points, int kind, size_t n_hypotheses, uint64_t seed,
                     uint32_t *samples);
/* Estimator::MinimalFit (ransac.h:138-162, 239-294, 354-417) for one sample on the HOST: pts = m x 3
 * doubles (m = 3 / 4 / 2), normals = m x 3 (cylinder only).  model: 8 doubles (first 4 / 7 = parameters),
 * *valid = MinimalFit's return.  Bit-identical to what the device computes for the same sample. */
int m3d_minimal_fit(int kind, const double *pts, const double *normals, double *model, uint8_t *valid);
int m3d_cloud_score_range(m3d_cloud *cloud, int kind, double threshold, const uint32_t *samples,
                          size_t begin, size_t end, uint32_t *counts, uint8_t *valid,
                          double *models);
/* Sequential sampler object = the RandomSampler of ransac.h:570 with an explicit seed; it records
 * every sample it has drawn (m3d_sampler_table(s, H) draws up to H hypotheses and returns the H x m
 * table).  m3d_cloud_score_shard scores ONE rank's share of hypotheses [begin,end) of that single
 * stream: the window is cut into slices of `slice` hypotheses, slice j belongs to rank j % world.
 * Every rank draws the whole window (identical tables everywhere), kernels for this rank's slices are
 * launched as soon as their samples exist, so drawing the other ranks' slices overlaps GPU scoring.
 * counts/valid receive this rank's records in increasing hypothesis order, *n_mine their number.
 * valid == NULL: counts[i] carries MinimalFit's return in bit 31 (counts are < 2^31) -- the 4-byte record the
 * ranks exchange; m3d_replay_chunk accepts the same form (valid == NULL). */
typedef struct m3d_sampler m3d_sampler;
m3d_sampler *m3d_sampler_create(size_t n_points, int kind, uint64_t seed);
void m3d_sampler_destroy(m3d_sampler *s);
size_t m3d_sampler_drawn(const m3d_sampler *s);
const uint32_t *m3d_sampler_table(m3d_sampler *s, size_t n_hypotheses);
int m3d_cloud_score_shard(m3d_cloud *cloud, m3d_sampler *sampler, double threshold, size_t begin,
                          size_t end, size_t slice, uint32_t world, uint32_t rank, uint32_t *counts,
                          uint8_t *valid, size_t *n_mine);
/* Serial-order error sum of EvaluateModel for ONE model (ransac.h:632-640), used to break
 * fitness ties exactly as the reference does.  *count is the inlier number, *error the sum. */
int m3d_cloud_exact_error(m3d_cloud *cloud, int kind, double threshold, const double *model,
                          uint64_t *count, double *error);
/* RefineModel (ransac.h:534-549) for a given pre-refinement model: inlier indices (ascending) and
 * GeneralFit applied in place to params.  Return 1/0 = GeneralFit's return.
 *
 * REFINED PARAMETERS, the accuracy contract of every entry point that returns them (m3d_fit_plane / m3d_fit_sphere,
 * m3d_cloud_fit, m3d_cloud_fit_batch, m3d_cloud_refine*, m3d_segment_plane_iterative*).  The reference answer is EXACT: for a
 * plane the closed form of ransac.h:164-211 (centred moment sums, the three determinants, the branch by the largest, the
 * `norm < 1e-8` failure) evaluated in rational arithmetic on the fit's own inliers; for a sphere the least-squares solution of
 * [2x 2y 2z 1] w = |p|^2 on them.  With err = the largest absolute difference of the four parameters,
 *     err <= max(32 err(fp64 restatement of the reference), F),   F = 16 * 2^-53 * max(1, max |inlier coordinate|, max |parameter|).
 * Where the exact closed form fails (fewer than 3 / 4 inliers, norm < 1e-8) the return is 0 and params is the best minimal model,
 * bit for bit.  A plane whose two largest determinants agree to 1e-9 is undecided: rounding picks the branch, and the result is
 * held to the nearer of the two branches' exact values, up to the sign of (a, b, c, d).  The sums are taken about a point
 * among the inliers -- a sample point of the winning hypothesis, or the inliers' mean -- never about a sphere's centre, which
 * lies a radius away from a cap of inliers (tests/test_gpu_generalfit.py, tests/test_generalfit.py). */
int m3d_cloud_refine(m3d_cloud *cloud, int kind, double threshold, double *params,
                     size_t *inliers, size_t *n_inliers);
/* Same, when the caller already knows the inlier count of `params` from the scoring pass (the record of the best
 * hypothesis, m3d_cloud_score_shard): the GeneralFit sums and the index-list copy are issued without waiting for
 * the compaction's own total, which is only checked at the end (a different total silently takes the ordinary
 * order).  expected_inliers < 0: unknown (= m3d_cloud_refine). */
int m3d_cloud_refine_expect(m3d_cloud *cloud, int kind, double threshold, double *params,
                            int64_t expected_inliers, size_t *inliers, size_t *n_inliers);
/* pcd_copy = pcd_copy->SelectByIndex(inliers, invert=true), src/iterative_plane_segmentation.cpp:33, on
 * the resident cloud: the inliers of `model` (distance < threshold, RefineModel's rule ransac.h:537-543)
 * leave the cloud, the rest keeps its order.  Afterwards every entry point works on the remaining
 * points, and the index lists it returns (m3d_cloud_fit, m3d_cloud_refine) keep referring to the cloud
 * AS CREATED, which is what SegmentPlaneIterative's callers need.  Clouds without normals only. */
int m3d_cloud_remove_inliers(m3d_cloud *cloud, int kind, double threshold, const double *model,
                             size_t *n_removed);
/* Sequential replay of the best-update / adaptive-stop rule (ransac.h:573-575,592-613) over
 * per-hypothesis (valid, count) records in index order; `rmse_cb` is called only for fitness ties.
 * Pure host logic, usable by distributed drivers after gathering counts.  valid == NULL: counts[i] carries
 * the valid flag in bit 31 (m3d_cloud_score_shard's packed form). */
typedef double (*m3d_rmse_fn)(void *user, size_t hypothesis_index);
typedef struct m3d_replay_state {
    double best_fitness, best_rmse;
    int64_t best_index;
    uint64_t best_count; /* inlier_num of the best hypothesis */
    uint64_t count, current_iteration, iterations;
    int32_t best_rmse_known, stopped;
} m3d_replay_state;
void m3d_replay_init(m3d_replay_state *st);
void m3d_replay_chunk(m3d_replay_state *st, size_t n_points, int kind, size_t max_iteration,
                      double probability, size_t begin, size_t end, const uint8_t *valid,
                      const uint32_t *counts, m3d_rmse_fn rmse_cb, void *user);

/* ---- segmentation::SegmentPlaneIterative, src/iterative_plane_segmentation.cpp:8-39 ----------- */
/* planes: 4 x max_clusters; cluster_offsets: max_clusters+1; cluster_indices: capacity n, indices
 * into the ORIGINAL cloud, ascending inside a cluster (SelectByIndex order).  Round r seeds its
 * sampler with *seed + r.  Returns 1; 0 when N < 3 (reference: warning + empty result, :13-17);
 * 2 when a round found no inlier (the reference would spin forever, :29-35). */
int m3d_segment_plane_iterative(const double *xyz, size_t n, double threshold, int max_iteration,
                                double min_ratio, const uint64_t *seed, int device,
                                size_t max_clusters, double *planes, size_t *cluster_offsets,
                                size_t *cluster_indices, size_t *n_clusters);
/* The same call returning the clusters' POINTS as well -- what the reference's function actually returns
 * (`cluster = pcd_copy->SelectByIndex(inliers)`, iterative_plane_segmentation.cpp:32,34: vector<pair<Vector4d, PointCloud>>).
 * cluster_points: capacity n x 3 doubles, may be NULL; receives the xyz of cluster_indices[i] at [3 i, 3 i + 3), gathered
 * on the device from the resident cloud and shipped in one copy (on the host SelectByIndex is a strided walk over the whole
 * input per big cluster: 135 ms of a 166 ms call on a 10 M-point room). */
int m3d_segment_plane_iterative_clouds(const double *xyz, size_t n, double threshold, int max_iteration,
                                       double min_ratio, const uint64_t *seed, int device, size_t max_clusters,
                                       double *planes, size_t *cluster_offsets, size_t *cluster_indices,
                                       double *cluster_points, size_t *n_clusters);

/* ---- registration::LeastSquareSolver::Solve, src/transform_estimation.cpp:49-66 (Eigen::umeyama) */
/* src, dst: n x 3.  T: row-major 4x4. */
int m3d_kabsch(const double *src, const double *dst, size_t n, int scaling, int device,
               double T[16]);

/* ---- registration::RANSACSolver::Solve, src/transform_estimation.cpp:124-164 ------------------ */
typedef struct m3d_reg_stats {
    double fitness, inlier_rmse;
    uint64_t validations;
    int64_t iterations, best_index, est_k;
    double ms_total;
    uint64_t ties;             /* equal-fitness comparisons decided during the replay (hypotheses the validation dropped early
                                * on their partial count or sum never get that far) */
    uint64_t exact_rmse_evals; /* of which needed the serial-order sum of squared distances */
    uint64_t lds_wave_hypotheses;    /* round 6: (256-point source tile, hypothesis) pairs whose record the validation's candidate cache made EXACT -- every
                                      * query answered from registers under a certificate (m3d_config.reg_cache; the field's name is round 2's, the
                                      * slot keeps the layout) */
    uint64_t global_wave_hypotheses; /* round 6: pairs it left as BOUNDS (count from above, sum from below); the neighbour-list walk evaluated those of
                                      * them whose hypothesis the pruning could not drop on the bounds (0 / 0: the cache did not run) */
    uint64_t nn_fp32_screen;         /* 1: the validation's neighbour search ran behind the fp32 screen (m3d_config.reg_fp32_screen and a
                                      * grid the screen admits: cell edge and offsets within fp32's reach) */
    uint64_t nn_screen_fallbacks;    /* queries whose runner-up lay within the rounding bound of the winner: decided by the fp64 walk */
} m3d_reg_stats;
/* corr_src/corr_dst: m index pairs (the std::pair<vector<size_t>,vector<size_t>> of the reference).
 * confidence: Open3D RANSACConvergenceCriteria::confidence_ (the reference always uses the default
 * 0.999, transform_estimation.cpp:160-161).  T: row-major 4x4.  stats may be NULL: the call then returns the pose only (all
 * RANSACSolver::Solve returns) and skips the pass that forms the winner's deterministic inlier_rmse. */
int m3d_registration_ransac(const double *src, size_t n_src, const double *dst, size_t n_dst,
                            const size_t *corr_src, const size_t *corr_dst, size_t m,
                            double threshold, int max_iter, double edge_length_threshold,
                            double confidence, const uint64_t *seed, int device, double T[16],
                            m3d_reg_stats *stats);

/* The same RANSAC as a session, cut into the steps a multi-GPU driver needs (hypotheses sharded, clouds and
 * grid replicated on every GPU).  Every rank creates an identical session (same seed):
 *   m3d_reg_begin_chunk   draws the triples of the next chunk of iterations, 3-point Kabsch + checkers;
 *                         *n_survivors = hypotheses that need validation.  Return 1 = chunk ready,
 *                         0 = the loop is over (call m3d_reg_finish), <0 error.
 *   m3d_reg_validate      (inlier count, sum of squared nearest distances) of survivors [s_begin, s_end) --
 *                         this rank's shard; s_begin must be a multiple of 64.
 *   m3d_reg_replay        sequential best-update / est_k rule over the chunk, given the records of ALL its
 *                         survivors (after the all-gather); identical inputs -> identical state on all ranks.
 * m3d_registration_ransac is exactly this loop with one shard. */
typedef struct m3d_reg m3d_reg;
m3d_reg *m3d_reg_create(const double *src, size_t n_src, const double *dst, size_t n_dst,
                        const size_t *corr_src, const size_t *corr_dst, size_t m, double threshold,
                        int max_iter, double edge_length_threshold, double confidence,
                        const uint64_t *seed, int device);
void m3d_reg_destroy(m3d_reg *reg);
int m3d_reg_begin_chunk(m3d_reg *reg, size_t *n_survivors);
int m3d_reg_validate(m3d_reg *reg, size_t s_begin, size_t s_end, uint32_t *counts, double *sums);
int m3d_reg_replay(m3d_reg *reg, const uint32_t *counts, const double *sums);
int m3d_reg_finish(m3d_reg *reg, double T[16], m3d_reg_stats *stats);

/* ---- misc3d::common::EstimateNormalsFromMap, src/normal_estimation.cpp:180-207 ---- */
/* xyz: h x w x 3 doubles, the organised point map row by row (pc->points_ with shape = (w, h)); a pixel is
 * valid iff its z is not NaN (:90).  k: window half-size ((2k+1)^2 neighbourhood, python default 5).
 * normals: h x w x 3 out; unit eigenvector of the smallest covariance eigenvalue, flipped towards view_point
 * (:165-171); NaN for invalid pixels (the reference leaves those uninitialised).  *ms_device (may be NULL):
 * device time of the three kernels.  The caller checks points == w * h like :187-191. */
int m3d_normals_from_map(const double *xyz, uint32_t w, uint32_t h, uint32_t k, const double view_point[3],
                         int device, double *normals, double *ms_device);

/* ---- misc3d::features::DetectBoundaryPoints, src/boundary_detection.cpp:68-113 -------- */
/* normals: n x 3 or NULL (then estimated from the same neighbourhood, :82-84).  search: 0 = KDTreeSearchParamKNN
 * (max_nn <= 128; radius ignored), 1 = KDTreeSearchParamRadius (radius), 2 = KDTreeSearchParamHybrid (radius,
 * max_nn <= 128) -- the python default is Hybrid(0.01, 30),
 * python/py_features.cpp:19.  angle_threshold in degrees (default 90).  indices: capacity n, written in
 * ascending order (the reference's order depends on thread timing); *k = their number.  Only the DIRECTION of a
 * normal matters, not its length or sign (the reference's basis has |u| = |n|, so there a normal that is not a unit
 * vector distorts the angles); a point whose normal has length zero or not finite (in double) is never flagged. */
int m3d_detect_boundary_points(const double *xyz, const double *normals, size_t n, int search, double radius,
                               int max_nn, double angle_threshold_deg, int device, size_t *indices, size_t *k);

/* ---- misc3d::preprocessing::FarthestPointSampling, src/filter.cpp:13-52 ------------------------------------------ */
/* indices (capacity num_samples) = the reference's samples, bit for bit: index 0 first, then at every step the lowest
 * index of the largest min-over-samples squared distance (3-element sum in the library's M3D_FP_ORDER association); when
 * no distance is > 0 the previous index repeats.  num_samples == 0: nothing; == n: 0 .. n-1; > n or < 0:
 * M3D_ERR_INVALID_ARG "Illegal number of samples: S, must <= point size: N" -- all three decided before any device is
 * touched.  n >= 2^31: M3D_ERR_INVALID_ARG.  stats may be NULL.  Re-entrant: concurrent calls take lanes of the device. */
#define M3D_FPS_PATH_SINGLE 1   /* one workgroup, all steps in one launch (small clouds) */
#define M3D_FPS_PATH_PRUNED 2   /* Hilbert-sorted 512-point tiles, one launch per sample, tiles skipped by a box bound */
#define M3D_FPS_PATH_DENSE 3    /* the same steps with every tile updated (measurement hook only: m3d_bench_fps_force_path) */
typedef struct m3d_fps_stats {
    double ms_total;            /* the call, host clock */
    double ms_device;           /* the sampling launches, HIP events (0 for the early cases) */
    int32_t path;               /* M3D_FPS_PATH_*, 0 = no device work */
    int32_t pad;
    uint64_t tiles_updated;     /* tile updates the steps ran (tiled paths) */
    uint64_t tile_steps;        /* tiles x steps: 1 - tiles_updated / tile_steps = the fraction pruned */
} m3d_fps_stats;
int m3d_farthest_point_sampling(const double *xyz, size_t n, int64_t num_samples, int device, size_t *indices,
                                m3d_fps_stats *stats);

/* ---- misc3d::preprocessing::CropROIPointCloud's indexing, src/filter.cpp:54-101 (host only, no device) ----------- */
/* n points of an organised cloud of shape (width, height), roi = (tl_x, tl_y, br_x, br_y): *k = (roi_w + 1) (roi_h + 1)
 * indices, indices[i] = (i / roi_w + tl_y) width + i % roi_w + tl_x with roi_w = br_x - tl_x, roi_h = br_y - tl_y -- the
 * reference's formula, rows roi_w wide, quirk included.  indices may be NULL (only *k).  n != width height:
 * M3D_ERR_INVALID_ARG "The size of point cloud is wrong."; roi_w <= 0 (the reference divides by it), roi_h < -1 or an
 * index outside [0, n) (the reference reads outside the cloud): M3D_ERR_INVALID_ARG. */
int m3d_crop_roi_indices(size_t n, int width, int height, int tl_x, int tl_y, int br_x, int br_y, size_t *indices,
                         size_t *k);

/* ---- open3d::geometry::PointCloud::VoxelDownSample (the first call of every example and of MultiScaleICP) --------- */
/* [RECALL] Open3D 0.15.1 PointCloud::VoxelDownSample / AccumulatedPoint, restated (tests/cpp/voxel_ref.c is the checker):
 *   1. voxel_size <= 0 or NaN: M3D_ERR_INVALID_ARG "[VoxelDownSample] voxel_size <= 0."
 *   2. min_bound / max_bound = the coordinate-wise min / max of the points; vmin = min_bound - voxel_size * 0.5,
 *      vmax = max_bound + voxel_size * 0.5; voxel_size * INT_MAX < max_c (vmax_c - vmin_c): M3D_ERR_INVALID_ARG
 *      "[VoxelDownSample] voxel_size is too small."
 *   3. voxel of point i, per coordinate: int(floor((p_c - vmin_c) / voxel_size)) -- one subtraction, one IEEE division
 *      (not a multiplication by a reciprocal: that moves points that lie on voxel faces), floor, int.
 *   4. per voxel the sums start at +0.0 and the members are added in ascending point index, one rounded fp64 addition
 *      per coordinate; normals likewise except that a normal with a NaN component is not added (the point still counts);
 *      colours likewise, none left out.
 *   5. out = sum / double(count) for point, normal (not re-normalised; the divisor counts the skipped ones) and colour.
 *   6. ORDER (ours; the reference iterates an unordered_map): voxels in ascending order of their lowest member index.
 *   7. deviations: a point with a non-finite coordinate is M3D_ERR_NON_FINITE, the message names the lowest such index
 *      (the reference's int(floor(NaN)) is undefined); a voxel_size of +inf and bounds whose vmin / vmax overflow are
 *      M3D_ERR_INVALID_ARG (the reference divides inf by inf); n == 0: M3D_OK, *m = 0.
 * The output equals that restatement bit for bit, in that order.  normals / colors: n x 3 or NULL (then their outputs
 * are not written and may be NULL).  out_xyz / out_normals / out_colors: capacity n rows; *m = the rows written.
 * out_first_index (capacity n, may be NULL): the lowest member index of output row j, strictly ascending.  point_to_voxel
 * (n, may be NULL): the output row of point i (what VoxelDownSampleAndTrace tells).  n > 2^30: M3D_ERR_INVALID_ARG.
 * On an error *m = 0 and the outputs are unspecified.  stats may be NULL.  Re-entrant: concurrent calls take lanes. */
#define M3D_VOXEL_PATH_PACKED 1 /* the three voxel indices fit 63 bits together: 64-bit keys in the hash table */
#define M3D_VOXEL_PATH_WIDE 2   /* any extent the reference accepts (3 x 31 bits): the table holds a member's index */
typedef struct m3d_voxel_stats {
    double ms_total;     /* the call, host clock */
    double ms_upload;    /* the cloud's host-to-device copies, HIP events on the lane's stream */
    double ms_device;    /* bounds, keys, grouping, ordered sums of every level (incl. the round trips for the bounds and m) */
    double ms_download;  /* the levels' rows (and trace arrays) device-to-host */
    uint64_t n_voxels;   /* rows written, all levels */
    int32_t path;        /* M3D_VOXEL_PATH_* of the last level, 0 = no device work */
    int32_t sort_passes; /* 8-bit passes of the stable sort, all levels */
} m3d_voxel_stats;
int m3d_voxel_down_sample(const double *xyz, const double *normals, const double *colors, size_t n, double voxel_size,
                          int device, double *out_xyz, double *out_normals, double *out_colors, size_t *out_first_index,
                          size_t *point_to_voxel, size_t *m, m3d_voxel_stats *stats);
/* n_levels voxel sizes, every level computed FROM THE ORIGINAL CLOUD (MultiScaleICP's shape, src/pipeline.cpp:937-938,
 * {v, v/2, v/4}): one upload, the bounds once.  out_xyz[l] .. point_to_voxel[l]: level l's arrays as above (the arrays of
 * pointers out_normals / out_colors / out_first_index / point_to_voxel may be NULL, as may their entries); m[l] = level
 * l's rows.  Every level equals the single call at that size bit for bit.  Every voxel size is checked before any
 * level runs. */
int m3d_voxel_down_sample_multi(const double *xyz, const double *normals, const double *colors, size_t n,
                                const double *voxel_sizes, size_t n_levels, int device, double *const *out_xyz,
                                double *const *out_normals, double *const *out_colors, size_t *const *out_first_index,
                                size_t *const *point_to_voxel, size_t *m, m3d_voxel_stats *stats);

/* ---- misc3d::segmentation::ProximityExtractor::Segment, src/proximity_extraction.cpp:51-190 ----------------------- */
/* The clusters are the connected components of the graph with an edge i - j when j is in i's radius neighbourhood
 * (d2 = (dx dx + dy dy) + dz dz <= radius^2, j != i) and the evaluator accepts (i, j, sqrt(d2)); a point with a non-finite
 * coordinate has no neighbours.  Components with min_size <= |C| <= max_size are kept (a larger one is dropped whole).
 * Order: size descending, ties by smallest member index ascending (the reference's unstable sort leaves it open); indices
 * within a cluster ascending.  cluster_offsets[0 .. *n_clusters] (capacity n + 1) delimit the clusters in cluster_indices
 * (capacity n).  labels (may be NULL, n entries): the rank of each point's cluster, *n_clusters for the points of no kept
 * cluster.  stats may be NULL.
 * Errors (M3D_ERR_INVALID_ARG): a normals evaluator with n_normals < n, "Index exceed size of data!"; a radius that is
 * negative or not finite; n >= 2^31.  n == 0: no clusters.  Re-entrant: concurrent calls take lanes of the device. */
#define M3D_PROX_DISTANCE 1         /* DistanceProximityEvaluator(dist):              dist < dist_thresh */
#define M3D_PROX_NORMALS 2          /* NormalsProximityEvaluator(normals, angle_deg)  acos(dot) vs Deg2Rad(angle_deg) */
#define M3D_PROX_DISTANCE_NORMALS 3 /* DistanceNormalsProximityEvaluator(normals, dist, angle_deg) */
typedef struct m3d_proximity_evaluator {
    int32_t kind;                   /* M3D_PROX_* */
    int32_t pad;
    double dist;                    /* distance threshold (DISTANCE, DISTANCE_NORMALS) */
    double angle_deg;               /* angle threshold in degrees (NORMALS, DISTANCE_NORMALS; < 0: unoriented normals) */
} m3d_proximity_evaluator;
typedef struct m3d_proximity_stats {
    double ms_total;                /* the call, host clock */
    double ms_device;               /* grid + union + flatten launches, HIP events */
    double ms_order;                /* the ordering of the components and the scatter of the indices, host clock */
    double cell_edge;               /* edge of the grid's cells (radius * 1.001 unless the 2^27-cell cap coarsened it) */
    uint64_t components;            /* connected components, kept or not */
} m3d_proximity_stats;
int m3d_proximity_segment(const double *xyz, const double *normals, size_t n_normals, size_t n, double radius,
                          const m3d_proximity_evaluator *ev, size_t min_size, size_t max_size, int device,
                          size_t *cluster_offsets, size_t *cluster_indices, size_t *n_clusters, size_t *labels,
                          m3d_proximity_stats *stats);
/* The nn_indices overload (:59-72): n_lists lists in CSR form (nn_offsets[0 .. n_lists], nn_indices); entry 0 of every
 * list is skipped (the reference's j = 1), edge i -> nn_indices[k] with dist = norm3(p_i - p_j) (Eigen's .norm()), the
 * clusters are the weakly connected components.  n_lists != n: M3D_ERR_INVALID_ARG "The number of input data size are not
 * equal!"; an index outside [0, n): M3D_ERR_INVALID_ARG.  Output as m3d_proximity_segment. */
int m3d_proximity_segment_nn(const double *xyz, const double *normals, size_t n_normals, size_t n, size_t n_lists,
                             const size_t *nn_offsets, const size_t *nn_indices, const m3d_proximity_evaluator *ev,
                             size_t min_size, size_t max_size, int device, size_t *cluster_offsets,
                             size_t *cluster_indices, size_t *n_clusters, size_t *labels, m3d_proximity_stats *stats);
/* Radius neighbour lists (j != i, d2 <= radius^2 as above), each sorted by (d2, index): the user-evaluator path of the
 * C++ / python ProximityExtractor.  offsets (n + 1 entries) always; *total = offsets[n].  nb_indices / nb_d2 (capacity
 * entries each) are filled when both are non-NULL and capacity >= *total -- call once with NULL to learn the size. */
int m3d_radius_neighbors(const double *xyz, size_t n, double radius, int device, size_t *offsets, uint32_t *nb_indices,
                         double *nb_d2, size_t capacity, size_t *total);

/* ---- misc3d::common::KNearestSearch, include/misc3d/common/knn.h, src/knn.cpp ------------------------------------- */
/* The EXACT answer that the reference's Annoy index approximates, for a resident dim x N matrix.
 *   Distance key: d2(q, r) = sum over k = 0 .. dim - 1 of (q[k] - r[k])^2, accumulated serially in dimension order in
 *     fp64 from +0.0, every subtraction, product and addition rounded (no FMA contraction): Annoy's euclidean_distance
 *     (annoylib.h:177-188), the matcher's order, and boundary detection's (dx dx + dy dy) + dz dz for dim 3.
 *   Order: ascending by (d2, row index) (Annoy partial_sorts pair<dist, index>).  A NaN d2 ranks after +inf, NaNs among
 *     themselves by index (the reference leaves this open); a NaN d2 is returned as the quiet NaN 0x7FF8000000000000.
 *   Count: a query gets kout = min(knn, N) results.
 *   Returned distance: sqrt(max(d2, 0)), correctly rounded -- bit-equal to libm's sqrt of the same d2 (Annoy's
 *     normalized_distance, annoylib.h:769-771); NaN stays NaN.
 *   SearchKNN (knn.cpp:103-113): -1 and empty lists when the index is empty, query.size() != dim or knn < 0.
 *   SearchHybrid (knn.cpp:115-139): the kout nearest; i = the first position with dist[i] > radius, or kout if none (a NaN
 *     distance or a NaN radius compares "not greater": inside); num = i - 1 results are kept -- the last in-radius
 *     neighbour is dropped -- and none when num == 0.  i == 0 (knn == 0, a negative radius, a nearest neighbour beyond
 *     the radius) wraps the reference's size_t and resize(SIZE_MAX) throws std::length_error: this API reports a count
 *     of -1 for that query (the C++ mirror throws std::length_error, python's single-query form raises ValueError).
 *   Search(param) (knn.cpp:81-101): Knn -> SearchKNN, Hybrid -> SearchHybrid, Radius -> -1.
 *   Limits, checked before any device is touched (M3D_ERR_INVALID_ARG): 1 <= dim <= 1024, 1 <= N < 2^31, data != NULL.
 *     knn has no upper cap.
 * Device paths ("k nearest neighbours"): GRID (dim 3, 1 <= kout <= 128: a density grid of about kout / 4 rows
 * per cell, built once per kout class on first use; shells around the query's cell until the kout-th pair is provably
 * final; queries with a non-finite coordinate take the tile path), TILE (any dim, 1 <= kout <= 128: brute force with
 * the rows staged through LDS, the database split across workgroups, the splits' lists merged in a second launch) and
 * SELECT (kout > 128: the tile path in pages of 128, each page strictly above the last pair of the previous one).  The
 * result does not depend on the path. */
typedef struct m3d_knn m3d_knn;
#define M3D_KNN_SEARCH_KNN 0     /* KDTreeSearchParam::SearchType::Knn */
#define M3D_KNN_SEARCH_HYBRID 2  /* KDTreeSearchParam::SearchType::Hybrid (Radius, 1, is not supported: -1) */
#define M3D_KNN_PATH_GRID 1
#define M3D_KNN_PATH_TILE 2
#define M3D_KNN_PATH_SELECT 3
typedef struct m3d_knn_stats {
    double ms_total;        /* the call, host clock */
    double ms_device;       /* first query upload to last result copy, HIP events (the last chunk's lane) */
    int32_t path;           /* M3D_KNN_PATH_* of the queries with finite coordinates (0: no device work) */
    int32_t launches;       /* kernel launches */
    uint64_t pair_dims;     /* (query, row) distances evaluated x dim, every page counted */
    uint64_t tile_queries;  /* queries that took the tile / select path on a grid-path call (non-finite coordinates) */
} m3d_knn_stats;
/* Uploads data (n rows of dim contiguous doubles: Eigen's column-major dim x N) to the device once.  NULL on failure
 * (m3d_last_error; *status, which may be NULL, = M3D_ERR_INVALID_ARG for the limits above, M3D_ERR_DEVICE otherwise).
 * The index is read-only afterwards: any number of threads may search it at once. */
m3d_knn *m3d_knn_create(const double *data, size_t n, int dim, int device, int *status);
/* Returns the device blocks to the pool.  No search on h may be running. */
void m3d_knn_destroy(m3d_knn *h);
size_t m3d_knn_size(const m3d_knn *h);
int m3d_knn_dim(const m3d_knn *h);
/* m queries (row-major m x dim).  search = M3D_KNN_SEARCH_KNN or M3D_KNN_SEARCH_HYBRID; knn >= 0 (M3D_ERR_INVALID_ARG
 * otherwise); radius is read by HYBRID only.  Outputs are row-major m x stride, stride >= kout = min(knn, N):
 * indices[q stride + j], dist[q stride + j] and d2 (may be NULL) for j < counts[q]; the rest of each row is padded with
 * SIZE_MAX / +inf.  counts[q] = kout (KNN), the hybrid count num or -1 (HYBRID, see above).  Queries are processed in
 * chunks of at most 16384 (tile, select) or 65536 (grid) queries, halved until the chunk's device scratch -- queries,
 * the splits' lists of one page, the merged page -- fits 256 MiB; a chunk of one query needs at most 0.4 MiB.  Re-entrant: concurrent searches on one index take lanes of its device.
 * stats may be NULL. */
int m3d_knn_search(const m3d_knn *h, const double *queries, size_t m, int search, int64_t knn, double radius, size_t stride,
                   size_t *indices, double *dist, double *d2, int64_t *counts, m3d_knn_stats *stats);

/* ---- fragment preprocessing: PreProcessFragments, src/pipeline.cpp:379-401 ----------------------------------------- */
/* EstimateNormals(Hybrid(2 voxel, 30)) when the fragment has no normals, OrientNormalsTowardsCameraLocation(), then
 * ComputeFPFHFeature(Hybrid(5 voxel, 100)) -- the producer of the descriptors that m3d_match_mutual_nn,
 * m3d_global_registration and m3d_register_fragment_pairs consume.  Open3D's source is in neither tree: the arithmetic
 * below is a [RECALL] of Open3D 0.15.1 (pipelines/registration/Feature.cpp, geometry/EstimateNormals.cpp,
 * PointCloud::OrientNormalsTowardsCameraLocation), as the ICP and the RANSAC registration are; THIS TEXT is the contract
 * (tests/cpp/fpfh_ref.c restates it in plain C).
 *
 * Neighbourhood (both calls; the same as m3d_detect_boundary_points): search = 0, KDTreeSearchParamKNN (the max_nn
 *   nearest) or 2, KDTreeSearchParamHybrid (the max_nn nearest among those with d2 < radius^2);
 *   d2 = (dx dx + dy dy) + dz dz in fp64, every operation rounded; the query point itself is included; neighbours are
 *   ordered by (d2, index); 1 <= max_nn <= 128.  A pair whose d2 is not finite is no neighbour pair: a point with a
 *   non-finite coordinate has no neighbours and is nobody's neighbour.  m = the number of neighbours found (self included).
 *   M3D_ERR_INVALID_ARG, all decided before any device is touched: search = 1 (Radius: unbounded lists are not
 *   supported, the message says so), any other search value, max_nn outside [1, 128], a Hybrid radius that is negative or
 *   NaN, n >= 2^31, a null array with n > 0.  n == 0: M3D_OK, nothing written.
 *
 * Normals.  m < 3: (0, 0, 1).  Otherwise the covariance in cumulant form, sums taken in neighbour order:
 *   s = sum (x, y, z, xx, xy, xz, yy, yz, zz) / m, C = E[ab] - E[a] E[b], and the unit eigenvector of its smallest
 *   eigenvalue by J3x3 (m3d_eig3.hpp).  Open3D's default is a closed-form solver whose roundings cannot be restated from
 *   memory: the DIRECTION is specified, not the bits.  A zero-length result becomes (0, 0, 1).
 *   orient != 0 (camera: 3 doubles), with v = camera - p: a zero normal becomes v / |v| ((0, 0, 1) when v is zero),
 *   any other normal is negated when n . v < 0.
 *
 * FPFH.  feature_out: n rows of 33 doubles = Eigen's column-major 33 x N (Feature::data_).
 *   Pair features of (p1, n1) with a neighbour (p2, n2): dp = p2 - p1, d = |dp|; d == 0: all features 0.
 *     a1 = n1 . dp / d, a2 = n2 . dp / d.  If acos(|a1|) > acos(|a2|): the roles of n1 and n2 are swapped, dp = -dp,
 *     f2 = -a2; else f2 = a1.  v = dp x n1; |v| == 0: all features 0; v /= |v|; w = n1 x v; f1 = v . n2;
 *     f0 = atan2(w . n2, n1 . n2).  Dot products and norms are 3-element reductions of the library's M3D_FP_ORDER.
 *     The acos of that comparison is the HOST libm's.  Estimated normals of neighbouring points often agree to an ulp, and
 *     two acos implementations may order such arguments differently, which swaps the frame and moves the pair to other
 *     bins.  The device therefore lists every point with a pair whose two (device) acos values are unequal arguments'
 *     results within 64 eps of each other, relative; the host evaluates the SPFH rows of those points with the same
 *     code and its own libm, and FPFH reads the rows after that (m3d_fpfh_stats.tie_points counts them).
 *   SPFH of point i with m > 1 (entry 0 of the list -- the point itself -- is skipped): incr = 100 / (m - 1); every
 *     other neighbour adds incr to the bins clamp(floor(11 (f0 + pi) / (2 pi))), 11 + clamp(floor(11 (f1 + 1) 0.5)),
 *     22 + clamp(floor(11 (f2 + 1) 0.5)), clamped to [0, 10].  m <= 1: a zero row.  (The device counts the pairs per
 *     bin in integers and multiplies by incr once: off the repeated addition by roundings of order 1e-14.)
 *   FPFH of point i with m > 1: over the same neighbours k >= 1 in list order, skipping d2[k] == 0:
 *     acc[j] += spfh[nb_k][j] / d2[k] (the SQUARED distance, as FLANN returns it), sum[j / 11] += the same value; then
 *     sum[g] = 100 / sum[g] where sum[g] != 0, and out[j] = acc[j] sum[j / 11] + spfh[i][j].  m <= 1: a zero row.
 *   So each of a row's three groups sums to 200 (100 when every weighted neighbour row is empty, 0 for an isolated point).
 *
 * Device ("FPFH"): one upload and one density grid per call (m3d_knn.hip's grid path with the cloud as its own
 * query set); the neighbour lists of a search stay in device memory, 12 bytes per pair, until SPFH and FPFH have read
 * them (a search whose lists would exceed 8 GiB is M3D_ERR_INVALID_ARG).  Re-entrant: concurrent calls take lanes. */
typedef struct m3d_fpfh_stats {
    double ms_total;        /* the call, host clock */
    double ms_device;       /* first launch to last launch, HIP events (uploads and result copies excluded) */
    double ms_upload;       /* grid build on the host + uploads, host clock */
    double ms_search;       /* the neighbour searches (+ the Hybrid cut), HIP events */
    double ms_normals;      /* normal estimation / orientation */
    double ms_spfh;
    double ms_fpfh;
    uint64_t pairs;         /* neighbour pairs processed: the sum of m over the points, every search counted */
    uint64_t pairs_seen;    /* (query, row) distances the searches evaluated */
    int32_t launches;       /* kernel launches */
    int32_t searches;       /* neighbour searches (0, 1 or 2) */
    uint64_t tie_points;    /* points whose SPFH row the host redid (a near tie of the two acos values, above) */
} m3d_fpfh_stats;
typedef m3d_fpfh_stats m3d_normals_stats;
/* open3d PointCloud::EstimateNormals(param) (+ OrientNormalsTowardsCameraLocation(camera) when orient != 0) for an
 * unorganised cloud.  normals_out: n x 3.  camera may be NULL when orient == 0.  stats may be NULL. */
int m3d_estimate_normals(const double *xyz, size_t n, int search, double radius, int max_nn, int orient,
                         const double camera[3], int device, double *normals_out, m3d_normals_stats *stats);
/* open3d ComputeFPFHFeature(cloud, param).  normals == NULL: M3D_ERR_INVALID_ARG "Failed because input point cloud has
 * no normal."  stats may be NULL. */
int m3d_compute_fpfh(const double *xyz, const double *normals, size_t n, int search, double radius, int max_nn, int device,
                     double *feature_out, m3d_fpfh_stats *stats);
/* PreProcessFragments for one fragment: normals by Hybrid(2 voxel_size, 30) only when normals_in == NULL, orientation
 * towards the origin always, FPFH by Hybrid(5 voxel_size, 100); one upload, one grid, both searches on the device.
 * normals_out (n x 3) receives the normals the descriptor was computed with; the result equals m3d_estimate_normals
 * followed by m3d_compute_fpfh bit for bit.  voxel_size must be positive and finite. */
int m3d_preprocess_fragment(const double *xyz, const double *normals_in, size_t n, double voxel_size, int device,
                            double *normals_out, double *feature_out, m3d_fpfh_stats *stats);

/* ---- point-to-point ICP refinement of the RANSAC pose ----------------------- */
/* open3d::pipelines::registration::RegistrationICP(source, target, max_correspondence_distance, init,
 * TransformationEstimationPointToPoint(), ICPConvergenceCriteria(relative_fitness, relative_rmse,
 * max_iteration)) as the reference's examples call it right after RANSACSolver::Solve
 * (examples/cpp/transform_estimation.cpp:82-86; defaults 1e-6, 1e-6, 30).  T_init: row-major 4x4 or NULL =
 * identity.  correspondences (n_src entries, may be NULL): target index of every source point, -1 = none
 * (Open3D's correspondence_set_). */
typedef struct m3d_icp_stats {
    double fitness;            /* correspondences / n_src */
    double inlier_rmse;        /* sqrt(sum d^2 / correspondences) */
    uint64_t correspondences;
    int32_t iterations;        /* ICP iterations executed */
    int32_t converged;         /* 1 = both relative criteria met before max_iteration */
    double ms_total;
} m3d_icp_stats;
int m3d_registration_icp(const double *src, size_t n_src, const double *dst, size_t n_dst,
                         double max_correspondence_distance, const double *T_init, int max_iteration,
                         double relative_fitness, double relative_rmse, int device, double T[16],
                         m3d_icp_stats *stats, int64_t *correspondences);

/* ---- point-to-plane ICP: LocalRefineMethod::Point2PlaneICP of MultiScaleICP, src/pipeline.cpp:949-955 ------------- */
/* RegistrationICP(source, target, max_correspondence_distance, init, TransformationEstimationPointToPlane(),
 * ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration)).  The arguments of m3d_registration_icp plus
 * dst_normals (n_dst x 3, used as given: not normalised).  The outer loop, stats and correspondences are those of
 * m3d_registration_icp; only ComputeTransformation differs.
 * [RECALL] Open3D 0.15.1 TransformationEstimationPointToPlane::ComputeTransformation, restated (tests/cpp/icp_ref.c is the
 * checker), over the correspondence set (i, j = nn[i]) with the moving point s as currently transformed:
 *   1. dst_normals == NULL: M3D_ERR_INVALID_ARG "TransformationEstimationPointToPlane and
 *      TransformationEstimationColoredICP require pre-computed normal vectors for target PointCloud."
 *      max_correspondence_distance <= 0 or NaN: M3D_ERR_INVALID_ARG "Invalid max_correspondence_distance." (checked first).
 *   2. r = (s - t_j) . n_j; J = [s x n_j, n_j] (6 values), cross = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0).
 *   3. JTJ = sum J J^T (21 distinct sums), JTr = sum J r (6 sums); the loss is L2 (weight 1).
 *   4. an empty correspondence set: the update is the identity.
 *   5. det(JTJ) (partial-pivot LU) not finite or |det| < 1e-6: the update is the identity (SolveLinearSystemPSD's check).
 *   6. otherwise x = LDLT(JTJ).solve(-JTr) and update = [Rz(x2) Ry(x1) Rx(x0) | x3, x4, x5] (TransformVector6dToMatrix4d).
 *   7. fitness and inlier_rmse are the Euclidean ones of GetRegistrationResultAndCorrespondences (nearest target point within
 *      the distance, lowest index on exact ties); the point-to-plane r^2 does not feed the stop rule.
 *   8. ORDER (ours): the sums are tree sums of a fixed shape -- equal bits from run to run -- not the serial sums of a
 *      one-thread loop: poses agree with the restatement to 1e-9, correspondence sets and iteration counts exactly on
 *      well-conditioned inputs.
 * Device ("Multi-scale ICP"): one fused launch per iteration (update, search, gather, 30 sums) and one small
 * launch that adds the workgroups' records; the 6 x 6 solve is the host's (misc3d_amd/csrc/m3d_icp_fp.hpp). */
int m3d_registration_icp_plane(const double *src, size_t n_src, const double *dst, const double *dst_normals, size_t n_dst,
                               double max_correspondence_distance, const double *T_init, int max_iteration,
                               double relative_fitness, double relative_rmse, int device, double T[16],
                               m3d_icp_stats *stats, int64_t *correspondences);

/* ---- point-to-plane ICP with L1 weights: RefineMethod::PointToPlane of PPFEstimator, src/ppf_estimation.cpp:937-990 ------
 * RegistrationICP(source, target, max_correspondence_distance, init, TransformationEstimationPointToPlane(L1Loss),
 * ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration)).  The arguments, refusals, empty-cloud results,
 * stats and correspondences of m3d_registration_icp_plane.  [RECALL] Open3D 0.15.1 robust_kernel.h: L1Loss::Weight(r) =
 * 1 / |r|, applied by ComputeJTJandJTr as JTJ += J w J^T, JTr += J w r.  Rules 1 - 8 of the plane call hold, with:
 *   L1. w = 1.0 / |r| per correspondence.
 *   L2. the record's 21 products are (J[a] w) J[b], its 6 values (J[a] w) r; the last slot stays r r (it feeds nothing).
 *   L3. r == 0: w is infinite and the record turns non-finite; rule 5 (a determinant that is not finite) then yields the
 *       identity update, as Open3D would: the next result repeats the last, which meets any positive stop criteria.
 * Device: icp_iter_k<IcpPlaneL1Rows>, the plane iteration's kernel template with the weighted rows; the small launch and the solve are shared. */
int m3d_registration_icp_plane_l1(const double *src, size_t n_src, const double *dst, const double *dst_normals, size_t n_dst,
                                  double max_correspondence_distance, const double *T_init, int max_iteration,
                                  double relative_fitness, double relative_rmse, int device, double T[16],
                                  m3d_icp_stats *stats, int64_t *correspondences);

/* ---- coloured ICP: LocalRefineMethod::ColoredICP of MultiScaleICP (the reference's default), src/pipeline.cpp:956-962 ------
 * RegistrationColoredICP(source, target, max_correspondence_distance, init, TransformationEstimationForColoredICP(
 * lambda_geometric), ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration)).  Arrays are row-major n x 3
 * doubles.  Colours are RGB as given (not clamped); normals are used as given (not normalised).
 * [RECALL] Open3D 0.15.1 colored_icp.cpp, restated (tests/cpp/colored_icp_ref.c is the checker).
 *
 * Colour gradients (InitializePointCloudForColoredICP), for target point k with position v, normal n:
 *   G1. The neighbour list L is the Hybrid search of "Neighbourhood" above with radius 2 max_correspondence_distance and
 *       max_nn 30 (m3d_color_gradient: the radius and max_nn it is given): at most max_nn nearest target points with
 *       d2 < r2, among the target points with three finite coordinates, sorted by (d2, original index).  The point itself
 *       is normally L[0].  A point with a non-finite coordinate has an empty list.
 *   G2. nn = |L|.  nn < 4: the gradient is (0, 0, 0).
 *   G3. The intensity of any point: I = ((c0 + c1) + c2) / 3.0.
 *   G4. For i = 1 .. nn - 1 (entry 0 is skipped whatever it is): p = xyz[L[i]]; s = (p - v) . n with the dot product
 *       (a0 b0 + a1 b1) + a2 b2; a_i = (p - s n) - v, component by component; b_i = I(L[i]) - I(k).
 *   G5. One last row: a = (nn - 1) n, b = 0.
 *   G6. AtA = sum a a^T (6 distinct sums) and Atb = sum a b, serial sums in row order, the row of G5 last; no contraction.
 *   G7. g = LDLT(AtA).solve(Atb), no determinant check (SolveLinearSystemPSD with its defaults): the pivoting and zero-pivot
 *       rules of the 6 x 6 solve at size 3 (misc3d_amd/csrc/m3d_icp_fp.hpp, one text for both).  A singular or non-finite
 *       system yields whatever those rules yield, stored as it is.
 *
 * One iteration (TransformationEstimationForColoredICP::ComputeTransformation), over the correspondence set:
 *   C1. lambda_geometric (Open3D's default 0.968): sg = sqrt(lambda), sp = sqrt(1 - lambda).
 *   C2. For a correspondence: s the source point as currently transformed; t, n, g the target's point, normal and gradient;
 *       Is the source point's intensity (it does not change under the pose); It the target's intensity.
 *   C3. Geometric row: e = (s - t) . n, r0 = sg e, J0 = sg [s x n, n] (cross product as in rule 2 of the plane call).
 *   C4. Photometric row: q = (s - e n) - t; I0 = g . q + It; m = -(g^T (I - n n^T)) with the nine entries written out
 *       (1.0 - n0 n0, -(n0 n1), ...), each component -((g0 M0c + g1 M1c) + g2 M2c); J1 = sp [s x m, m]; r1 = sp (Is - I0).
 *   C5. The record has the 30 slots of the plane call: count, Euclidean d2, the 21 products J0a J0b + J1a J1b, the 6 values
 *       J0a r0 + J1a r1, r0 r0 + r1 r1.  The loss is L2.
 *   C6. The rest is the plane call's rules 4 - 8 unchanged: the identity for an empty set or a determinant that is not finite
 *       or below 1e-6 in magnitude, the same solve of the record, the outer loop and stop rule on the Euclidean fitness and
 *       rmse, lowest index on exact ties, tree sums of a fixed shape (equal bits from run to run).
 *
 * M3D_ERR_INVALID_ARG, all before any device work, in this order: max_correspondence_distance <= 0 or NaN ("Invalid
 * max_correspondence_distance."); dst_normals == NULL (the plane call's text); src_colors or dst_colors == NULL
 * ("TransformationEstimationForColoredICP requires colors for the source and the target PointCloud."); lambda_geometric
 * outside [0, 1] or NaN ("lambda_geometric must be in [0, 1].").  T receives the initial pose on every refusal.
 * Empty clouds: as in the plane call (no device needed, the first repeat converges).
 * Device ("Coloured ICP"): color_gradient_k once per call, then one fused launch per iteration
 * (icp_iter_k<IcpColoredRows>) and the small launch that adds the workgroups' records. */
/* G1 - G7 alone: out_gradient n x 3.  max_nn in [1, 128], radius >= 0. */
int m3d_color_gradient(const double *dst, const double *dst_normals, const double *dst_colors, size_t n, double radius,
                       int max_nn, int device, double *out_gradient);
int m3d_registration_icp_colored(const double *src, const double *src_colors, size_t n_src, const double *dst,
                                 const double *dst_normals, const double *dst_colors, size_t n_dst,
                                 double max_correspondence_distance, double lambda_geometric, const double *T_init,
                                 int max_iteration, double relative_fitness, double relative_rmse, int device, double T[16],
                                 m3d_icp_stats *stats, int64_t *correspondences);

/* open3d::pipelines::registration::GetInformationMatrixFromPointClouds(source, target, max_dist, T): the
 * acceptance test of ReconstructionPipeline::GlobalRegistration, src/pipeline.cpp:818-824.
 * info: 6 x 6 row-major; info[35] == *n_correspondences (may be NULL). */
int m3d_information_matrix(const double *src, size_t n_src, const double *dst, size_t n_dst,
                           double max_correspondence_distance, const double *T, int device, double info[36],
                           uint64_t *n_correspondences);

/* ---- ReconstructionPipeline::MultiScaleICP, src/pipeline.cpp:927-982 -------------------------------------------------
 * What RegisterFragmentPair (:754-763: {voxel}, {50}) and RefineFragmentPair (:686-697: {v, v/2, v/4}, {50, 30, 15}) call.
 * Per level l: both clouds down-sampled with voxel_sizes[l] FROM THE ORIGINAL CLOUDS by the voxel contract above (target
 * normals are the per-voxel means, not re-normalised), then ICP with ICPConvergenceCriteria(1e-6, 1e-6, max_iters[l]) seeded
 * with the previous level's pose (level 0: T_init, NULL = identity) and max_correspondence_distance at every level (the
 * reference passes config.voxel_size * 1.4, :936).  After the last level info = GetInformationMatrixFromPointClouds(src, dst,
 * voxel_sizes[last] * 1.4, T) on the original clouds (:975-979).  The result equals m3d_voxel_down_sample_multi,
 * m3d_registration_icp / m3d_registration_icp_plane and m3d_information_matrix chained by the caller, bit for bit.
 * method: PipelineConfig::LocalRefineMethod.  src_normals: n_src x 3 or NULL (not read by methods 0 and 1).
 * T: 4 x 4 row-major, info: 6 x 6 row-major.  levels: n_levels records or NULL.
 * M3D_ERR_INVALID_ARG, all before any device work: n_levels == 0 (the reference returns an uninitialised matrix); method 2
 * or 3 (not accelerated: the message says so) or any other value; method 1 without dst_normals (rule 1 above); a voxel
 * size the voxel contract's rule 1 rejects, whatever its level; max_correspondence_distance <= 0; 2^30 points or more.
 * The whole call runs on one lane of the device.  Re-entrant: concurrent calls take lanes. */
#define M3D_REFINE_POINT2POINT_ICP 0
#define M3D_REFINE_POINT2PLANE_ICP 1
#define M3D_REFINE_COLORED_ICP 2      /* needs colours: m3d_multi_scale_icp_colored (refused here) */
#define M3D_REFINE_GENERALIZED_ICP 3  /* not accelerated */
typedef struct m3d_multi_scale_icp_level {
    uint64_t n_src, n_dst;   /* rows of the level's down-sampled clouds */
    m3d_icp_stats icp;       /* the level's ICP */
    double ms_down_sample;   /* both clouds' level, host clock (level 0 carries the two uploads and the bounds) */
    double ms_icp;           /* the level's ICP call: upload of the level, grid, iterations */
    double ms_information;   /* the information matrix (last level only) */
} m3d_multi_scale_icp_level;
int m3d_multi_scale_icp(const double *src, const double *src_normals, size_t n_src, const double *dst,
                        const double *dst_normals, size_t n_dst, const double *voxel_sizes, const int *max_iters,
                        size_t n_levels, double max_correspondence_distance, int method, const double *T_init, int device,
                        double T[16], double info[36], m3d_multi_scale_icp_level *levels);

/* MultiScaleICP with LocalRefineMethod::ColoredICP (:956-962): the arguments of m3d_multi_scale_icp without `method`, plus both
 * clouds' colours (n x 3) and lambda_geometric.  Every level is formed by the voxel contract with colours (both clouds) and
 * normals (target); the result equals m3d_voxel_down_sample_multi, m3d_registration_icp_colored and m3d_information_matrix
 * chained by the caller, bit for bit.  Errors as m3d_multi_scale_icp's, plus missing colours and lambda_geometric outside
 * [0, 1] (the texts of m3d_registration_icp_colored).  One lane for the whole call. */
int m3d_multi_scale_icp_colored(const double *src, const double *src_normals, const double *src_colors, size_t n_src,
                                const double *dst, const double *dst_normals, const double *dst_colors, size_t n_dst,
                                const double *voxel_sizes, const int *max_iters, size_t n_levels,
                                double max_correspondence_distance, double lambda_geometric, const double *T_init, int device,
                                double T[16], double info[36], m3d_multi_scale_icp_level *levels);

/* ---- ReconstructionPipeline::GlobalRegistration (Ransac method), src/pipeline.cpp:790-828, and its caller's shape: one
 * std::thread per fragment pair, src/pipeline.cpp:428-439 ----------------------------------------------
 * match (ANNMatcher::Match, :800-802) -> RANSACSolver(1.4 voxel_size).Solve (:806-807) -> pose.isIdentity(1e-8) ? (true,
 * pose, I6) (:814-816) -> GetInformationMatrixFromPointClouds (:818-820) -> info(5,5) / min(Ns, Nt) < 0.3 ? (false, pose,
 * I6) : (true, pose, info) (:821-825).  The whole pair runs on ONE lane of the device; the two clouds are uploaded once and
 * serve the solver and the information matrix.
 * feat_*: one descriptor of `dim` contiguous doubles per point (Feature::data_, Eigen dim x N column-major).
 * max_iter / edge_length_threshold: RANSACSolver's (defaults 100000 / 0.9, transform_estimation.h:121-123); confidence:
 * Open3D RANSACConvergenceCriteria's (0.999).  seed: NULL = std::random_device.
 * Returns M3D_OK = (true, ...), M3D_FALSE = (false, pose, I6), < 0 = the reference throws (fewer than 3 points) / device error.
 * T: 4 x 4 row-major, info: 6 x 6 row-major; both always written (identity on error). */
typedef struct m3d_global_reg_stats {
    uint64_t n_matches;              /* mutual pairs the matcher returned */
    uint64_t n_info_correspondences; /* info(5,5): correspondences within 1.4 voxel_size under the pose (0 when not evaluated) */
    int32_t identity_shortcut;       /* 1: pose.isIdentity(1e-8) ended the call (:814-816) */
    int32_t device, lane;            /* where the pair ran */
    int32_t reserved_;
    double ms_match, ms_ransac, ms_info, ms_total;   /* host clock */
    m3d_reg_stats ransac;
} m3d_global_reg_stats;
int m3d_global_registration(const double *src, size_t n_src, const double *dst, size_t n_dst, const double *feat_src,
                            const double *feat_dst, int dim, double voxel_size, int max_iter, double edge_length_threshold,
                            double confidence, const uint64_t *seed, int device, double T[16], double info[36],
                            m3d_global_reg_stats *stats);
/* BuildPoseGraphForScene's loop over fragment pairs (src/pipeline.cpp:428-439: one std::thread per pair, joined): pair k
 * runs on devices[k % n_dev]; every device works on up to `inflight` (<= 0: m3d_config.lanes) of its pairs at a time, each on a
 * lane of its own, so one pair's uploads and host-side steps (cross-check, RANSAC replay) run under another's kernels.
 * Pairs are independent: no collective, results identical to n_pairs calls of m3d_global_registration with the same seeds.
 * Every pair's rc / T / info / stats are written; the call returns the first failed pair's (negative) code, else M3D_OK. */
typedef struct m3d_fragment_pair {
    const double *src, *dst;           /* n x 3 */
    size_t n_src, n_dst;
    const double *feat_src, *feat_dst; /* n x dim */
    uint64_t seed;
    int32_t has_seed;                  /* 0: std::random_device */
    int32_t rc;                        /* out: M3D_OK accepted / M3D_FALSE rejected / < 0 error */
    double T[16], info[36];            /* out */
    m3d_global_reg_stats stats;        /* out */
} m3d_fragment_pair;
int m3d_global_registration_batch(m3d_fragment_pair *pairs, size_t n_pairs, int dim, double voxel_size, int max_iter,
                                  double edge_length_threshold, double confidence, const int *devices, int n_dev,
                                  int inflight);

/* The same loop as the reference holds its data (preprocessed_fragment_lists_ / fragment_features_ + pairs (s, t) by index,
 * src/pipeline.cpp:415-440): every fragment a device needs is uploaded to it ONCE, by the first pair that asks for it, and
 * stays resident for the call -- a fragment of the all-pairs loop is otherwise uploaded n - 1 times.  Pair k runs on
 * devices[k % n_dev], `inflight` pairs at a time per device.  Results: those of m3d_global_registration on the same arrays
 * and seeds.  Returns the first failed pair's (negative) code, else M3D_OK; every pair carries its own rc. */
typedef struct m3d_fragment_view {
    const double *xyz;  /* n x 3 */
    const double *feat; /* n x dim */
    size_t n;
} m3d_fragment_view;
typedef struct m3d_pair_result {
    int32_t s, t;                /* in: fragment indices (source, target) */
    int32_t has_seed;            /* in: 0 = std::random_device */
    int32_t rc;                  /* out: M3D_OK accepted / M3D_FALSE rejected / < 0 error */
    uint64_t seed;               /* in */
    double T[16], info[36];      /* out */
    m3d_global_reg_stats stats;  /* out */
} m3d_pair_result;
int m3d_register_fragment_pairs(const m3d_fragment_view *frags, size_t n_frags, int dim, m3d_pair_result *pairs,
                                size_t n_pairs, double voxel_size, int max_iter, double edge_length_threshold,
                                double confidence, const int *devices, int n_dev, int inflight);

/* ---- pose_estimation::RayCastRenderer, src/ray_cast_renderer.cpp ------------------------------------------------------
 * Depth, instance and primitive maps of a list of posed triangle meshes seen by a pinhole camera at the origin looking
 * along +z: what RayCastRenderer::CastRays computes through Open3D's RaycastingScene (Embree, CPU only).  Bit parity with
 * Embree is not a goal (it promises no order among equal hits and no operation order); the contract below is ours, follows
 * the reference wherever the reference is visible, and is checked bit for bit against tests/cpp/raycast_ref.c.  Facts about
 * Open3D marked [RECALL] are from memory of 0.15.  The arithmetic of rules 1-4 is misc3d_amd/csrc/m3d_raycast_fp.hpp.
 *   1. CAMERA.  width W, height H, fx, fy, cx, cy (fp64).  The ray of pixel (x, y), row-major index y W + x, starts at
 *      (0, 0, 0) with direction d = (fp32(((x + 0.5) - cx) / fx), fp32(((y + 0.5) - cy) / fy), 1.0f): computed in fp64, rounded
 *      once, NOT normalised, so a hit's t is its z-depth ([RECALL] CreateRaysPinhole; app/label_maker/mixed/helper.py:145 and
 *      GetPointCloud's rays[:, 3:] * t_hit rely on it).
 *   2. SCENE.  Mesh g (geometry id g = its position in the list, [RECALL] AddTriangles returns ids in order) has fp64
 *      vertices, triangles as three int32 vertex indices, and a row-major 4 x 4 fp64 pose T whose last row is not read.  A
 *      vertex becomes fp32(((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3]) per row r: fp64, every operation rounded
 *      separately (no contraction), rounded once to fp32.  From there on everything is fp32 with every operation rounded
 *      separately, division and square root correctly rounded and subnormals kept (hipcc's defaults for gfx950; the library
 *      is built with -ffp-contract=off).  A transformed vertex that is not finite in fp32: M3D_ERR_NON_FINITE (the message
 *      names the vertex and the frame), the outputs are then unspecified.
 *   3. ONE (RAY, TRIANGLE) PAIR.  Moeller-Trumbore in this order: e1 = v1 - v0, e2 = v2 - v0, p = d x e2, det = e1 . p,
 *      s = -v0, u = (s . p) / det, q = s x e1, v = (d . q) / det, t = (e2 . q) / det, with a x b = (a1 b2 - a2 b1,
 *      a2 b0 - a0 b2, a0 b1 - a1 b0) and a . b = (a0 b0 + a1 b1) + a2 b2.  A hit needs det != 0, u >= 0, v >= 0,
 *      u + v <= 1 and 0 < t < +inf; both faces are hit; NaN fails every comparison.  It needs in addition, with the box of
 *      the triangle (coordinate-wise min / max of its three fp32 vertices): slab(ray, box) = [a, b] non-empty (a <= b) and
 *      t >= lower(box) = a - 2^-16 b.  slab: per axis with d != 0 the values lo (1 / d) and hi (1 / d), the smaller-side one
 *      near, the other far (by the sign of d); a = the maximum of the near values and 0, b = the minimum of the far values and
 *      +inf, a NaN product (0 x inf) constraining nothing; an axis with d == 0 fails the box unless lo <= 0 <= hi.  Rounding is
 *      monotone and min / max of fp32 values are exact, so for boxes A inside B the slab of B contains the slab of A and
 *      lower(B) <= lower(A) in floating point: a traversal that skips a node whose slab fails or whose lower exceeds the
 *      best t so far loses no hit and no tie.  The clause rejects no Moeller-Trumbore hit of the reference's example scene
 *      (DESIGN.md "Ray casting").
 *   4. ONE RAY.  The hit with the smallest t wins; on equal t the lowest geometry id, then the lowest primitive id (the
 *      triangle's index within its mesh): the answer depends on neither the hierarchy nor the traversal order.  Outputs per
 *      pixel: t_hit (fp32, +inf on a miss), geometry_ids and primitive_ids (uint32, 0xFFFFFFFF on a miss, [RECALL] Open3D's
 *      INVALID_ID), primitive_normals (3 x fp32): c = (v1 - v0) x (v2 - v0) of the transformed triangle, l2 = c . c, the
 *      normal c / sqrt(l2) per component, not flipped towards the ray; (0, 0, 0) on a miss and when l2 is 0 or not finite.
 *   5. ERRORS, all decided before any device work.  n_meshes == 0: no error, the call returns M3D_FALSE and
 *      m3d_last_error() is "No mesh is provided." (:67-69: a warning, CastRays returns false).  n_meshes != n_poses:
 *      M3D_ERR_SIZE_MISMATCH "The number of meshes and poses are not matched." (:71).  M3D_ERR_INVALID_ARG: a vertex index
 *      outside [0, n_vertices); a non-finite vertex, pose entry or intrinsic; width or height < 1; fx or fy == 0; a corner
 *      pixel's direction not finite in fp32; 2^31 triangles or pixels, 2^32 vertices or 2^32 - 1 meshes, or more.  A mesh with
 *      zero triangles is legal and keeps its id.  Without a device: M3D_ERR_DEVICE; there is no CPU path.
 * poses: n_frames x n_poses row-major 4 x 4 matrices, frame-major -- the label makers' shape (app/label_maker/real/
 * generate_labels.py:153-177: the same meshes at new poses, frame after frame): the meshes are uploaded once and the frames run
 * back to back on one stream.  Outputs are laid out [frame][pixel] (n_frames x H x W entries, x 3 for the normals); any of
 * the four may be NULL.  n_frames == 0: M3D_OK, nothing written.  stats may be NULL.  Re-entrant: concurrent calls take
 * lanes of the device. */
typedef struct m3d_raycast_mesh {
    const double *vertices;   /* n_vertices x 3 */
    size_t n_vertices;
    const int32_t *triangles; /* n_triangles x 3 vertex indices */
    size_t n_triangles;
} m3d_raycast_mesh;
typedef struct m3d_raycast_stats {
    double ms_total;       /* host clock, entry to return */
    double ms_upload;      /* HIP events: the meshes and the poses to the device */
    double ms_build;       /* ... transform, sort, hierarchy, all frames */
    double ms_traverse;    /* ... the traversal, all frames */
    double ms_download;    /* ... the maps to the host */
    uint64_t n_triangles;  /* of the list */
    uint64_t n_nodes;      /* of one frame's hierarchy: 2 n_triangles - 1 */
    uint64_t n_rays;       /* n_frames x H x W */
    uint64_t pair_tests;   /* rule-3 tests run, all frames (n_rays x n_triangles without the hierarchy) */
    uint64_t nodes_visited; /* internal nodes visited, all frames */
} m3d_raycast_stats;
int m3d_raycast_pinhole(const m3d_raycast_mesh *meshes, size_t n_meshes, const double *poses, size_t n_poses, size_t n_frames,
                        int width, int height, double fx, double fy, double cx, double cy, int device, float *t_hit,
                        uint32_t *geometry_ids, uint32_t *primitive_ids, float *primitive_normals, m3d_raycast_stats *stats);

/* ---- registration::ANNMatcher::Match, src/correspondence_matching.cpp:52-84 ------------------- */
/* feat_*: Eigen MatrixXd dim x N column-major = N descriptors of dim contiguous doubles.
 * method: 0 FLANN, 1 ANNOY (correspondence_matching.h MatchMethod); both run the exact mutual
 * nearest-neighbour search on the GPU.  out_*: capacity n_src.  *k = number of matches. */
int m3d_match_mutual_nn(const double *feat_src, size_t n_src, const double *feat_dst, size_t n_dst,
                        int dim, int method, int n_trees, int device, size_t *out_src,
                        size_t *out_dst, size_t *k);
/* Diagnostics: number of queries of the calling thread's last m3d_match_mutual_nn call whose reduced-precision
 * screen was inconclusive (candidate list overflow / fp32 range) and that were redone by exact brute force. */
uint64_t m3d_match_last_fallbacks(void);

/* ---- multi-GPU: hypotheses sharded, points replicated ----------------------------------
 * The hypothesis loop of ransac.h:571-613 carries one dependency across iterations, the best-model update
 * (:592-613).  Sharded, every rank (one GPU each) holds a replica of the cloud and an identically seeded sampler,
 * scores a contiguous slice of every window of the ONE hypothesis stream, and a single all-gather per window
 * exchanges the 4-byte (MinimalFit's return << 31 | inlier count) records; every rank then replays the same
 * sequence, so best hypothesis, iteration count, inlier list and parameters are identical on every rank and equal
 * to the one-GPU result for any number of ranks.  No point ever crosses the links.
 *
 * m3d_comm is the exchange.  Three ways to get one:
 *   m3d_comm_create_rccl   one process per GPU: rank 0 calls m3d_comm_unique_id, the launcher's own channel
 *                          (torch.distributed store, MPI_Bcast, a file) hands the 128 bytes to every rank, every
 *                          rank calls m3d_comm_create_rccl(id, world, rank, device) -- collective, like
 *                          ncclCommInitRank.  The all-gather then runs as ncclAllGather on the library's stream,
 *                          in place on the device record array (RCCL over xGMI; librccl is bound at run time).
 *   m3d_comm_create_host   the caller supplies the all-gather over host buffers (MPI_Allgather, gloo, tests).
 *   m3d_comm_create_local  `world` communicators for `world` threads of this process, one device each
 *                          (m3d_segment_plane_iterative_multi uses it).
 * A communicator is used by one thread at a time; all ranks must make the same sequence of sharded calls. */
typedef struct m3d_comm m3d_comm;
#define M3D_COMM_ID_BYTES 128
int m3d_comm_unique_id(uint8_t id[M3D_COMM_ID_BYTES]);
m3d_comm *m3d_comm_create_rccl(const uint8_t id[M3D_COMM_ID_BYTES], int world, int rank, int device);
/* recv: world x bytes_per_rank, rank-major.  Return 0 on success. */
typedef int (*m3d_allgather_fn)(void *user, const void *send, void *recv, size_t bytes_per_rank);
m3d_comm *m3d_comm_create_host(int world, int rank, m3d_allgather_fn fn, void *user);
int m3d_comm_create_local(int world, m3d_comm **comms /* world handles out */);
void m3d_comm_destroy(m3d_comm *comm);
int m3d_comm_world(const m3d_comm *comm);
int m3d_comm_rank(const m3d_comm *comm);
uint64_t m3d_comm_collectives(const m3d_comm *comm); /* exchanges made so far */

/* m3d_cloud_fit (RANSAC::FitModel, ransac.h:482-516) with the hypothesis loop sharded over the ranks of `comm`.
 * Every rank passes its own replica of the cloud and the SAME kind / threshold / max_iteration / probability;
 * seed == NULL: rank 0 draws one from std::random_device and shares it.  Outputs are written on every rank.
 * comm == NULL is m3d_cloud_fit.  stats->hypotheses_scored counts this rank's share. */
int m3d_cloud_fit_sharded(m3d_cloud *cloud, m3d_comm *comm, int kind, double threshold, size_t max_iteration,
                          double probability, const uint64_t *seed, double *params, size_t *inliers,
                          size_t *n_inliers, m3d_stats *stats);
/* m3d_segment_plane_iterative with every round's hypothesis loop sharded: each rank uploads the same cloud to its
 * own `device`, removes the same inliers from its replica after every round (no point traffic), and returns the
 * same clusters. */
int m3d_segment_plane_iterative_sharded(const double *xyz, size_t n, double threshold, int max_iteration,
                                        double min_ratio, const uint64_t *seed, int device, m3d_comm *comm,
                                        size_t max_clusters, double *planes, size_t *cluster_offsets,
                                        size_t *cluster_indices, size_t *n_clusters);
/* The same from ONE process that drives n_dev GPUs (the `devices[], n_dev` form): a thread and a
 * replica per device, records exchanged through host memory.  devices must be distinct ordinals.  n_dev == 1 is
 * m3d_segment_plane_iterative on devices[0]. */
int m3d_segment_plane_iterative_multi(const double *xyz, size_t n, double threshold, int max_iteration,
                                      double min_ratio, const uint64_t *seed, const int *devices, int n_dev,
                                      size_t max_clusters, double *planes, size_t *cluster_offsets,
                                      size_t *cluster_indices, size_t *n_clusters);
int m3d_fit_multi(int kind, const double *xyz, const double *normals, size_t n, double threshold,
                  size_t max_iteration, double probability, const uint64_t *seed, const int *devices, int n_dev,
                  double *params, size_t *inliers, size_t *n_inliers, m3d_stats *stats);
/* m3d_registration_ransac with the validation of every chunk's surviving hypotheses sharded (contiguous runs of
 * 64-hypothesis groups per rank, one all-gather of (count, sum d^2) per chunk, identical replay everywhere). */
int m3d_registration_ransac_sharded(const double *src, size_t n_src, const double *dst, size_t n_dst,
                                    const size_t *corr_src, const size_t *corr_dst, size_t m, double threshold,
                                    int max_iter, double edge_length_threshold, double confidence,
                                    const uint64_t *seed, int device, m3d_comm *comm, double T[16],
                                    m3d_reg_stats *stats);

/* ---- tunables ---------------------------------------------------------------------------------------------------
 * Every knob of the library, read ONCE from the environment on first use (variable names in brackets) and
 * replaceable at run time.  None changes a result: they select between code paths that produce identical output
 * (the test-suite runs them against each other) or set launch geometry.  m3d_set_config may be called while other threads
 * compute: a call works with the settings as they were when it took its lane (a snapshot per call), the new ones apply to calls
 * that start afterwards.  Returns M3D_ERR_INVALID_ARG for score_mfma / score_waves4 / compact_one_pass != 0: the
 * variants those switches selected were measured slower and removed (commit 71d1ee3 is the last that contains them; the
 * measurements: profiles/r04_score_mfma.txt, r04_score_waves4.txt, r04_compact_one_pass.txt). */
typedef struct m3d_config {
    int32_t dense_scoring;          /* [M3D_DENSE=1]        1: score every (tile, hypothesis) pair (score_k) instead of the culled path */
    int32_t speculative_refine;     /* [M3D_SPEC=0]         default 1: probability-1 fits start RefineModel on the device's own pick */
    int32_t lead_hypotheses;        /* [M3D_LEAD]           default 128 (multiple of 64): hypotheses counted first for the pruning incumbent */
    int32_t score_groups_per_block; /* [M3D_GPB]            default 8: 64-hypothesis groups per scoring workgroup (1..64); the fp32-screen kernels take twice that for
                                       windows of 192 groups and more, and at most 16 */
    int32_t score_min_workgroups;   /* [M3D_SCORE_MIN_WGS]  default 8192: small chunks are cut finer to reach this many workgroups */
    int32_t dense_workgroups;       /* [M3D_SCORE_WGS]      default 8192: workgroup target of the dense kernel */
    int32_t reg_neighbour_lists;    /* [M3D_REG_NL=0]       default 1: per-cell 3x3x3 neighbour lists for the registration validation */
    int32_t reg_prune;              /* [M3D_REG_PRUNE=0]    default 1: bound-and-prune of validations against earlier chunks */
    int32_t match_brute;            /* [M3D_MATCH_BRUTE=1]  1: fp64 brute-force matcher (no screen) */
    int32_t match_fp32_screen;      /* [M3D_MATCH_SCREEN=fp32] 1: fp32 VALU screen instead of the split-fp16 MFMA screen */
    int32_t pool_limit_mb;          /* [M3D_POOL_MB]        default 4096: released device blocks parked per device for re-use (0 = none) */
    int32_t kernel_timing;          /* [M3D_KERNEL_TIMING=1] default 0; 1: HIP events attached to every scoring launch (hipExtLaunchKernel: the
                                       launch's own start / stop times, no barrier packets) fill m3d_stats.ms_score_kernel /
                                       score_launches (bench.py switches it on: ~4 us per C2 fit); ms_score becomes a host clock around the scoring phase */
    int32_t reg_sorted_lists;       /* [M3D_REG_SORTED=0]   default 1: x-sorted neighbour lists, side columns cut off by the x-distance */
    int32_t score_fp32_screen;      /* [M3D_SCORE_SCREEN=0] default 1: planes and spheres are counted by score_screen_k (packed-fp32 screen with a
                                       rounding bound in front of the exact fp64 test: identical counts); 0: fp64 only (score_mask_k) */
    int32_t cull_fp32;              /* [M3D_CULL_FP32=0]    default 1: the box tests of the culled path run in fp32 with outward-rounded margins
                                       (cull_tiles32_k, and cull_hyp32_k for windows of 128 groups and more: conservative, identical results); 0: fp64 box tests
                                       (cull_tiles_k); 2: fp32, always with a lane per tile (cull_tiles32_k: the tests' switch) */
    int32_t reg_fp32_screen;        /* [M3D_REG_SCREEN=0]   default 1: the nearest-neighbour search of the registration validation finds its
                                       candidate in fp32 on 8-byte list entries (16-bit fixed-point coordinates over the cell's 3-cell
                                       block + the entry's position, rounding bound) and evaluates the winner in fp64; a query whose
                                       runner-up is within the bound takes the fp64 walk: identical distances */
    int32_t sorted_tombstones;      /* [M3D_TOMBSTONES=0]   default 1: a segmentation round that removes a sliver of the cloud kills its inliers
                                       in place in the Hilbert-sorted copy (x = NaN: never an inlier; the screen masks the lane) instead
                                       of partitioning the copy; a real compaction follows when an eighth of the copy is dead */
    int32_t score_mfma;             /* retired, must be 0 (the slot is kept for the layout) */
    int32_t score_mfma_groups;      /* retired, ignored (reads back as 0) */
    int32_t score_waves4;           /* retired, must be 0 */
    int32_t score_waves4_groups;    /* retired, ignored (reads back as 0) */
    int32_t score_phases;           /* [M3D_SCORE_PHASES]   default -1 = 3 for cylinders, 0 for planes and spheres (measured: m3d_cull_kernels.hip,
                                       "PHASED scoring"); 2 / 3 (every kind): a window that has an incumbent is counted on a quarter of the
                                       tiles, re-pruned with what every hypothesis collected (count so far + 512 per tile it can still touch
                                       against the incumbent: exact), (3: counted on a second quarter, re-pruned,) and only the survivors
                                       see the rest; 0: one launch over all tiles */
    int32_t compact_one_pass;       /* retired, must be 0 */
    int32_t plane_bound;            /* [M3D_PLANE_BOUND=0]  default 1: plane fits -- and since round 5 cylinder fits: the shell over a tile is a slab up to a
                                       sagitta -- with an incumbent prune with a per-tile HISTOGRAM upper bound of
                                       every (tile, hypothesis) pair's inlier count (tile_frames_k / plane_bound_k, m3d_bound.hip) instead of
                                       512 per touched tile, where that pays (windows of >= 8192 hypotheses on tiles x hypotheses >= 1.5e7, measured: m3d_fit.cpp
                                       bound_pays; 2: whatever the size, and sphere fits too); same results, fewer hypotheses counted point by point.  (Fields are
                                       only ever appended, the offsets of existing fields do not move -- ADVICE r3) */
    int32_t lanes;                  /* [M3D_LANES]          default 4 (1..8): calls a device runs side by side -- every lane has its own streams and
                                       scratch, a call holds one from entry to return, host threads are dealt lanes in the order they arrive
                                       (a single-threaded caller lives on lane 0); 1 = one call at a time per device (rounds 1-4) */
    int32_t wait_spin_us;           /* [M3D_SPIN_US]        default 500: the end of a fit's device work is waited for by polling a completion word in
                                       page-locked memory (the runtime's wait wakes the caller 10-20 us late) for at most this many
                                       microseconds, then by hipStreamSynchronize (a blocked thread, no core burnt: long calls, hosts with
                                       more fitting threads than cores); 0 = the runtime's wait only */
    int32_t prestream;              /* [M3D_PRESTREAM=0]    default 1: MinimalFit + box tests of a fit's chunk k + 1 run on a second stream under the
                                       scoring launches of chunk k; 0: everything on the lane's main stream (same records) */
    int32_t chunk_cap;              /* [M3D_CHUNK_CAP]      default 24576 (1024..262144, multiple of 64): hypotheses per chunk of the culled path */
    int32_t first_chunk;            /* [M3D_FIRST_CHUNK]    default 2048 (0 = off): length of the short first chunk of a fit of several chunks (the
                                       incumbent that prunes the rest) */
    int32_t reg_cells_per_radius;   /* [M3D_REG_K]          default 4 (1..16): cells per search radius of the registration validation's grid for a target of
                                       200 000 points and more; for a smaller target the value is scaled by the cube root of the size ratio and
                                       rounded, so any integer of 1 .. the value may result (3 at the default for 48 800 to 134 000 points) */
    int32_t match_pipeline;         /* [M3D_MATCH_PIPELINE] default 1: a match of two large host matrices (>= 65 536 rows each) uploads them in slices (two of
                                       the queries, four of the database) and scans block (i, j) while the next slice is on the link (same result:
                                       tests/test_gpu_match_sliced.py) -- when the call is alone on the device (other calls' kernels fill the gap
                                       anyway); 0: both matrices uploaded first; 2: sliced whatever the size and the company (the tests' switch) */
    int32_t reg_cache;              /* [M3D_REG_CACHE]      default 1: a registration RANSAC that validates many hypotheses keeps, per source point, the 32
                                       target points nearest to its position under the incumbent pose in registers and answers a hypothesis'
                                       nearest-neighbour queries from them wherever a certificate holds (every other target point provably
                                       farther); the other (tile, hypothesis) pairs take the neighbour-list walk.  Same counts, sums and pose
                                       (m3d_reg_cache.hip).  0: the walk only; 2: the cache as soon as an incumbent exists (the tests' switch) */
    int32_t device_aliases;         /* [M3D_DEVICE_ALIASES] default 0; N > 0: device ordinals 0 .. max(N, physical devices) - 1 are valid, ordinal d living
                                       on physical device d % physical -- each with its own lanes, streams, scratch, free lists and
                                       resident tables, as a further physical device would have.  For executing the multi-device entry
                                       points (devices[] forms, m3d_fit_multi, m3d_register_fragment_pairs) on a box with fewer GPUs than
                                       the code path wants: it exercises the dealing, the per-device state and the in-process exchange,
                                       NOT peer traffic or RCCL across devices.  m3d_device_count() then returns the logical count (<= 16) */
    int32_t lanes_eager;            /* [M3D_LANES_EAGER]    default 2 (1..lanes): lanes whose compute streams a device's FIRST call creates; the others appear when
                                       a call needs them.  Streams take hardware queues in creation order, and a lane created after another lane's
                                       copy / pre stream shares a queue with it (its calls take turns with that lane's): a process that runs many
                                       calls side by side (m3d_cloud_fit_batch over four lanes, fragment pairs in flight) sets 4 before its first
                                       call; a single-threaded caller keeps 2 (its fits of several chunks are 10-20 % faster that way) */
    int32_t list_mask;              /* [M3D_LIST_MASK]      default 1: a plane / sphere fit that returns its inlier list into page-locked memory
                                       (m3d_host_alloc) gets it from the device as a bit mask -- 1 bit per point instead of 8 bytes per inlier
                                       over the host link -- and the host writes the indices, with up to 8 threads (the caller's + a
                                       process-wide pool of helpers, woken when the fit queues its compaction, spinning at most
                                       wait_spin_us); N >= 2: the same with at most N writers (<= 16); 0: the device writes the list */
    int32_t mask_early;             /* [M3D_MASK_EARLY=0]   default 1: with list_mask, the compaction's counting launch stores the tile counts beside
                                       its mask rows and the launch behind it announces them ("mask ready") before it folds the moments:
                                       the host writes the list under that launch and waits for its completion word afterwards; 0: the
                                       host waits for the completion word first (same list, same parameters) */
    int32_t ref_bound;              /* [M3D_REF_BOUND]      default 1: a one-GPU plane fit whose first chunk has a lead pass also bins every tile's
                                       points by their signed distance to the lead's best plane (ref_hist_tile, in the lead_fold_keep_k
                                       launch), and plane_bound_k takes the smaller of its two bounds per (tile, hypothesis) pair -- where
                                       plane_bound engages (bound_pays); 2: whatever the size (forces plane_bound's launch too: the tests);
                                       0: off.  Same results, fewer hypotheses counted point by point */
} m3d_config;
void m3d_get_config(m3d_config *out);
int m3d_set_config(const m3d_config *in);

/* ---- PPF voting: the table and the vote of misc3d::pose_estimation::PPFEstimator, src/ppf_estimation.cpp -----------------
 * The two device hot paths of the class: CalcHashTable (:603-640) with GenerateModelPCNeighbor (:1236-1253) behind
 * m3d_ppf_model_create, VotingAndGetPose (:399-524) with CalcLocalMaximum (:1170-1234) behind m3d_ppf_vote.  Both take
 * ALREADY SAMPLED points with unit normals (row-major n x 3 doubles).  ClusterPoses / PoseAverage, the refinement and the
 * scoring are below ("PPF pose clustering"), the EdgePoints mode and PreprocessEstimate below this block ("PPF voting,
 * EdgePoints mode", m3d_ppf_prepare_scene); PreprocessTrain is m3d_ppf_prepare_model ("PPF model preprocessing"), the PPFEstimator class the host mirrors' (python pose_estimation.PPFEstimator, include/misc3d/pose_estimation/ppf_estimation.h).
 * The text below is the contract; tests/cpp/ppf_ref.c restates it in serial C.
 *
 * MODEL (Train, :537-570, VotingMode::SampledPoints).  points[n], normals[n], diameter, r_min and m3d_ppf_params.
 *   M1. angle_num = round(pi / angle_step) + 1, alpha_model_num = 2 angle_num - 1, dist_num = round(1 / rel_sample_dist) + 1,
 *       dist_step = diameter rel_sample_dist, hash_table_size = angle_num^3 dist_num (:538-542).
 *   M2. centroid = the serial sum of the points in index order, divided by n; the points are centred by it (:551-560).
 *   M3. tmg[i] = CalcTNormal2RegionX(p_i, n_i) (:674-697), on the host with its libm: u = (0, n_z, -n_y), scaled by 1 / |u|
 *       when |u| > 1e-6, else (0, 1, 0); h = acos(n_x) / 2 (n_x clamped to [-1, 1]: the reference's acos is NaN beyond);
 *       quaternion (cos h, 0, sin h u_y, sin h u_z) through QuatToMat; translation -((R_r0 x + R_r1 y) + R_r2 z).
 *   M4. per ordered pair i != j: d = p_j - p_i, d2 = (dx dx + dy dy) + dz dz, u = d / sqrt(d2) component-wise,
 *       f0 = acos((n_i.x u.x + n_i.y u.y) + n_i.z u.z), f1 the same with n_j, f2 = acos(n_i . n_j) (sums in that order), f3 =
 *       sqrt(d2) (CalcPPF, :642-653); quantised round(f / angle_step), round(f3 / dist_step) (:655-661); cell = q0 + q1
 *       angle_num + q2 angle_num^2 + q3 angle_num^3 (HashPPF, :663-666); alpha = atan2(-z, y) of tmg[i] p_j with y, z =
 *       ((R_r0 x + R_r1 y) + R_r2 z) + t_r (CalcAlpha, :699-704); quant_alpha = round((alpha + pi) / angle_step) (:632).
 *   M5. the table is flat: cell_offsets[hash_table_size + 1] and entries (i, quant_alpha), within a cell in ascending (i, j)
 *       (the reference's order is the arrival order of a `critical` section).
 *   M6. the neighbour list of point i (GenerateModelPCNeighbor, radius 0.5 r_min): every j, i included, with d2 <
 *       (0.5 r_min)^2, ascending -- d2 < r^2 is the library's neighbourhood rule.
 * VOTE (:399-524).  scene points[m], normals[m], reference[n_ref] (indices into the scene).  Per reference position s:
 *   V1. tsg = CalcTNormal2RegionX of the reference point, on the host as M3.
 *   V2. neighbours: the scene points with d2 < r_min^2 (the reference point itself is one); n_searched = their number.
 *   V3. the gate: nothing is voted and nothing reported unless n_searched > size_t(n 0.2) (:412, :450).
 *   V4. a neighbour with sqrt(d2) < min_dist_thresh r_min && n_1 . n_0 > cos(min_angle_thresh) is left out (:456-459).
 *   V5. quantize_alpha and the quantised feature as M4 (pair: reference point -> neighbour, frame tsg); SpreadPPF (:706-743):
 *       the cells q + shift, shifts {-1, 0, +1} on the distance, the first k of {-1, 0, +1} on each angle (k = 2 in faster
 *       mode, else 3), a shifted bin outside its range dropped: 24 or 81 cells in the interior.
 *   V6. each (cell, quantize_alpha) votes at most once per reference position (flags_b); every entry (i, quant_alpha) of a
 *       voting cell increments accumulator[i alpha_model_num + (quant_alpha - quantize_alpha + alpha_model_num) %
 *       alpha_model_num].
 *   V7. CalcLocalMaximum exactly: per row the best circular three-window sum, strict > (the first maximum wins); nothing
 *       unless the largest is >= size_t(n 0.2); threshold size_t(max 0.8); rows in ascending order, a row above the
 *       threshold whose max_flag is still set clears the max_flags of its neighbours it is not smaller than (itself
 *       included) -- also when it is not a maximum itself -- and is reported when none of its neighbours is larger.
 *   V8. output: the maxima (reference position, model index, alpha index, votes) in ascending (reference position, model
 *       index) -- the reference's order is arrival order -- and per maximum the pose tsg^-1 Rx(alpha index angle_step)
 *       tmg[model index] (:497-515; the inverse is the rigid one, the products are the host's).  These are the
 *       reference's pose_list for the CENTRED model; m3d_ppf_model_centroid gives the centroid.
 * WHERE THE REFERENCE IS UNDEFINED:
 *   U1. `1 << quantize_alpha` is an int shift, undefined beyond 31 bins: the flags are 64-bit here and alpha_model_num > 64
 *       is M3D_ERR_INVALID_ARG (so is alpha_model_num < 3, where the windows of V7 read past a row, and
 *       hash_table_size >= 2^24).
 *   U2. a pair with d2 == 0 would normalise a zero vector: it is skipped, in the table and in the vote.
 *   U3. a quantised distance >= dist_num would index past the table and past dist_shift_lut_: the pair is skipped (a d2 that
 *       is not finite falls here).
 *   U4. acos of a dot product just outside [-1, 1] is NaN in the reference: here it falls in the end bin.  y == 0 and z == 0
 *       in M4's alpha counts as alpha = 0.
 *   U5. a non-finite coordinate or normal is M3D_ERR_INVALID_ARG; so are n < 2, n > 65535, n_ref == 0, a reference index
 *       >= m, and a diameter, r_min or parameter that is not positive and finite.
 *   U6. the accumulator holds 16-bit counts and cannot overflow: for a fixed row and alpha index each table entry
 *       contributes at most once per reference position, so every count is <= n - 1 <= 65534.
 * HOW BINS ARE DECIDED.  No bin is decided by a transcendental function on the device (misc3d_amd/csrc/m3d_ppf_fp.hpp, the
 * one text host and device compile, without contraction): round(acos(x) / step) = the number of k with x <= cos((k + 1/2)
 * step); round(sqrt(d2) / dist_step) = the number of k with d2 >= ((k + 1/2) dist_step)^2; the alpha bin = the number of
 * edge directions (cos, sin)((b + 1/2) step - pi) the vector (y, -z) has passed, by the sign of -z and of one cross product
 * per edge.  The edge tables are computed once on the host and uploaded.  Every output of the device is an integer, so host
 * and device agree bit for bit; the contract differs from the reference's libm only for a pair within a few ulp of an edge.
 * DEVICE ("PPF voting").  Table: one pass over the n^2 pairs writes keys, the shared stable radix sort orders
 * them by (cell, i, j), two passes give offsets and entries (scratch: 16 bytes a pair, capped at 4 GiB -- n <= 16383, beyond it
 * M3D_ERR_DEVICE); a count, a scan and a fill give the neighbour lists.  Vote: one workgroup per reference position, its
 * accumulator in LDS whenever it fits (M3D_PPF_PATH_LDS: (n alpha_model_num + 1) / 2 words <= 140 KiB, 2 312 rows at 31 bins),
 * else in device memory (M3D_PPF_PATH_DEVICE) -- a function of (n, alpha_model_num) only; the once-per-(cell, bin) rule by
 * atomic-or on a flag array per workgroup in device scratch, cleared by revisiting the touched cells; the call's scratch
 * stays within 256 MiB.  Nothing in the result depends on scheduling or on the order of the scene points. */
typedef struct m3d_ppf_model m3d_ppf_model;
typedef struct m3d_ppf_params {
    double rel_sample_dist;   /* training_param_.rel_sample_dist, 0.05 */
    double angle_step;        /* voting_param_.angle_step in RADIANS (the reference's 12 degrees = pi / 15) */
    double min_dist_thresh;   /* voting_param_.min_dist_thresh, 1 / 3 */
    double min_angle_thresh;  /* voting_param_.min_angle_thresh in RADIANS (30 degrees = pi / 6) */
    int32_t faster_mode;      /* voting_param_.faster_mode, 1 */
    int32_t reserved;
} m3d_ppf_params;
#define M3D_PPF_PATH_LDS 1
#define M3D_PPF_PATH_DEVICE 2
#define M3D_ERR_CAPACITY (-9) /* m3d_ppf_vote: more maxima than the caller's buffers hold; *n_maxima = the needed count */
typedef struct m3d_ppf_table_info {
    uint64_t table_size;      /* hash_table_size */
    uint64_t n_entries;       /* pairs in the table */
    uint64_t n_neighbors;     /* total length of the neighbour lists */
    int32_t angle_num, alpha_model_num, dist_num;
    int32_t path;             /* M3D_PPF_PATH_* the vote takes for this model */
} m3d_ppf_table_info;
typedef struct m3d_ppf_vote_stats {
    int32_t path;                  /* M3D_PPF_PATH_* */
    uint32_t launches;             /* kernel launches of the call */
    uint32_t groups;               /* workgroups of the vote (each takes every groups-th reference position) */
    uint32_t reserved;
    uint64_t neighbours_visited;   /* the sum of n_searched */
    uint64_t increments;           /* accumulator increments */
    double ms_device;              /* HIP events around the call's device work */
    double ms_total;               /* wall clock of the call */
} m3d_ppf_vote_stats;
void m3d_ppf_default_params(m3d_ppf_params *out);
/* params == NULL: the defaults.  NULL + *status (may be NULL) = M3D_ERR_* on failure.  The model is read-only afterwards:
 * any number of threads may vote on it at once (each call takes a lane). */
m3d_ppf_model *m3d_ppf_model_create(const double *points, const double *normals, size_t n, double diameter, double r_min,
                                    const m3d_ppf_params *params, int device, int *status);
void m3d_ppf_model_destroy(m3d_ppf_model *model);
size_t m3d_ppf_model_size(const m3d_ppf_model *model);
int m3d_ppf_model_centroid(const m3d_ppf_model *model, double centroid[3]);
/* Reads the table back.  Every array may be NULL (call once with info alone for the sizes): cell_offsets[table_size + 1],
 * entry_i / entry_alpha[n_entries], nbr_offsets[n + 1], nbr_indices[n_neighbors], tmg[n x 16] (row-major 4 x 4 each). */
int m3d_ppf_model_table(const m3d_ppf_model *model, m3d_ppf_table_info *info, uint32_t *cell_offsets, uint16_t *entry_i,
                        uint8_t *entry_alpha, uint32_t *nbr_offsets, uint32_t *nbr_indices, double *tmg);
/* V1 - V8.  The four result arrays hold `capacity` entries each, poses (may be NULL) capacity x 16 doubles (row-major 4 x 4).
 * *n_maxima = the number of maxima.  More than capacity: M3D_ERR_CAPACITY, nothing is written to the arrays, and
 * *n_maxima says what capacity the call needs. */
int m3d_ppf_vote(const m3d_ppf_model *model, const double *scene_points, const double *scene_normals, size_t m,
                 const size_t *reference, size_t n_ref, size_t capacity, size_t *n_maxima, uint32_t *ref_pos,
                 uint32_t *model_index, uint32_t *alpha_index, uint32_t *votes, double *poses, m3d_ppf_vote_stats *stats);

/* ---- PPF voting, EdgePoints mode: VotingMode::EdgePoints of PPFEstimator, src/ppf_estimation.cpp -------------------------
 * The reference's second voting mode, for flat parts whose shape is in their boundary: the table pairs the model sample with
 * the model's EDGE points (Train, :572-593, CalcHashTable with b_same_pointset == false), the vote pairs a scene sample point
 * with the scene's edge points (Estimate, :319-328).  Only what differs from M1 - M6, V1 - V8, U1 - U6 and K1 - K8 is said
 * here; tests/cpp/ppf_ref.c restates both modes in serial C (its edge arrays are optional: null means SampledPoints).
 *   E1. Inputs: points[n], normals[n] (the model sample), edge_points[n_e], edge_normals[n_e], diameter, r_min, params.  Sizes
 *       as M1.  The centroid is M2's, from the n sample points alone; BOTH sets are centred by it.
 *   E2. tmg[i] as M3, for the sample points.
 *   E3. One candidate per ordered pair (i in the sample, j in the edges), all n n_e of them, EQUAL INDICES INCLUDED (the two
 *       sets are different sets).  Features and bins as M4 with p_j, n_j from the edge set and alpha from tmg[i] applied to
 *       the edge point.  U2 applies and matters: a pair with d2 == 0 is skipped -- both samplers of the reference pick
 *       original points, so an edge point that coincides with a sample point is normal.  U3 applies.
 *   E4. The layout is M5's: within a cell the entries (i, quant_alpha) are in ascending (i, j).
 *   E5. The neighbour lists are M6's over the sample points.
 *   E6. The vote takes the scene sample points[m], normals[m], reference[n_ref] (indices into the sample) and the scene's edge
 *       points[m_e], normals[m_e].  tsg as V1 from the reference point.  The neighbours are the scene EDGE points with d2 <
 *       r_min^2 of the reference point; n_searched is their number (the reference point is in general not one of them).
 *   E7. The gate: vote only when n_searched > size_t(n_e 0.2) (refered_model_num = n_e, :450); maxima need max_votes >=
 *       size_t(n_e 0.2) (:1204).
 *   E8. V4 - V8 otherwise unchanged: n accumulator rows, the sample's neighbour lists, the output order.
 *   E9. m3d_ppf_estimate_edges runs K1 - K7 unchanged: the ICP is the centred model sample against the scene SAMPLE (:339),
 *       not against the edges.  K8 uses expected = (ratio n) n, without the 0.25 (:358-364: both counts are the sample's size
 *       in either mode, the reduction factor applies to SampledPoints only).
 * WHERE THE REFERENCE IS WRONG.  It builds a centred copy of the dense model sample (:573-584) and never uses it: :588-589
 * select the edge points from the UNCENTRED dense_model_sample_.  Its table so pairs centred sample points with uncentred
 * edge points and is right only for a model whose centroid is the origin.  E1 centres both sets (tests/test_ppf_edge.py shows
 * a known pose recovered with E1 and lost with the edge set left uncentred).
 * LIMITS.  1 <= n_e <= 65535: U6's argument gives every count <= n_e, so the 16-bit counters hold, and a row's three-window
 * sum is <= 3 x 65535 and fits rowinfo.  n n_e <= 2^28 pairs (the 4 GiB sort scratch), beyond it M3D_ERR_DEVICE.  1 <= m_e <
 * 2^31.  A non-finite edge point or normal is M3D_ERR_INVALID_ARG.  The 256 MiB scratch rule counts m_e scanned points and
 * the n_ref reference points: only those are uploaded.  The accumulator path is still a function of (n, alpha_model_num).
 * MODE MISMATCHES.  m3d_ppf_vote / m3d_ppf_estimate on an edge model, and the _edges calls on a sampled model, are
 * M3D_ERR_INVALID_ARG with a message that names the model's mode, decided before any device is touched. */
/* E1 - E5.  The model holds the sample with its frames, neighbour lists, centroid and ICP source, and the edge table; the
 * same-set table is not built.  Otherwise as m3d_ppf_model_create. */
m3d_ppf_model *m3d_ppf_model_create_edges(const double *points, const double *normals, size_t n, const double *edge_points,
                                          const double *edge_normals, size_t n_edge, double diameter, double r_min,
                                          const m3d_ppf_params *params, int device, int *status);
/* n_e; 0 for a SampledPoints model (m3d_ppf_model_table reports the edge table of an edge model) */
size_t m3d_ppf_model_edge_size(const m3d_ppf_model *model);
/* E6 - E8; results, M3D_ERR_CAPACITY and stats exactly as m3d_ppf_vote */
int m3d_ppf_vote_edges(const m3d_ppf_model *model, const double *scene_points, const double *scene_normals, size_t m,
                       const size_t *reference, size_t n_ref, const double *scene_edge_points,
                       const double *scene_edge_normals, size_t m_edge, size_t capacity, size_t *n_maxima, uint32_t *ref_pos,
                       uint32_t *model_index, uint32_t *alpha_index, uint32_t *votes, double *poses, m3d_ppf_vote_stats *stats);

/* ---- PPFEstimator::PreprocessEstimate, src/ppf_estimation.cpp:243-278: a host composition of calls of this library ---------
 * on one device, in the reference's order:
 *   1. points with a non-finite coordinate are dropped, order kept, their normals' rows with them (RemoveNonFinitePoints);
 *      none left: M3D_ERR_INVALID_ARG "There is no scene point clouds." (so is n == 0).
 *   2. normals == NULL: m3d_estimate_normals(Hybrid, radius = calc_normal_relative diameter, max_nn 30, no orientation).
 *   3. NormalConsistent (include/misc3d/utils.h:130-144) on the host without contraction: a normal is negated when
 *      (p.x n.x + p.y n.y) + p.z n.z > 0; then s = (n.x n.x + n.y n.y) + n.z n.z and each component is divided by sqrt(s) when
 *      s > 0.
 *   4. m3d_voxel_down_sample(points, normals, dist_step) -> sample_xyz / sample_normals, *n_sample rows.
 *   5. dist_step_dense > 0: m3d_voxel_down_sample(points, normals, dist_step_dense) -> dense_xyz / dense_normals, *n_dense
 *      rows, and m3d_detect_boundary_points(dense, dense normals, Hybrid, the radius of step 2, max_nn = pts_num, 90 degrees) ->
 *      edge_indices (ascending, into the dense sample), *n_edges.  dist_step_dense <= 0 or NaN: no edge part, *n_dense =
 *      *n_edges = 0 and the three dense arrays may be NULL.
 * The voxel means' normals are NOT re-normalised (rule 5 of the voxel contract, as in the reference): they go to the vote as
 * they are.  Every output array has capacity n rows.  Errors are those of the composed calls. */
int m3d_ppf_prepare_scene(const double *xyz, const double *normals, size_t n, double diameter, double calc_normal_relative,
                          double dist_step, double dist_step_dense, int pts_num, int device, double *sample_xyz,
                          double *sample_normals, size_t *n_sample, double *dense_xyz, double *dense_normals, size_t *n_dense,
                          size_t *edge_indices, size_t *n_edges);

/* ---- PPF model preprocessing: PPFEstimator::PreprocessTrain, src/ppf_estimation.cpp:206-241 with :1018-1160 -----------------
 * ORIENTATION (m3d_orient_normals_mst).  The reference's priority-queue walk (CalcModelNormalAndSampling, :1083-1148) is lazy
 * Prim: the first done neighbour of the point it pops is that point's parent in the minimum spanning tree of the radius
 * graph, rooted at the seed ("PPF model preprocessing").  The device builds that tree by Boruvka rounds
 * (m3d_orient.hip), the host walks it once (m3d_ppf_train.hpp).  tests/cpp/ppf_train_ref.c restates the heap walk in serial C.
 *   O1. Vertices are the n points; all coordinates must be finite (M3D_ERR_INVALID_ARG otherwise).  {i, j} is an edge iff
 *       i != j and d2(i, j) < radius radius, d2 = (dx dx + dy dy) + dz dz without contraction (m3d_proximity_fp.hpp's prox_d2;
 *       nanoflann's strict cut-off, the library's neighbourhood rule K3).  d2 is symmetric bit for bit.
 *   O2. Edges are ordered by (d2, min(i, j), max(i, j)); T is the minimum spanning forest under that order.  The reference's
 *       own order is looser at ties (sqrt merges distinct d2, its sort and heap are not stable): this build differs from it
 *       only where its result depends on its standard library.
 *   O3. parent[seed] = -1; for every other point of the seed's component, parent is the neighbour on the tree path to the
 *       seed; parent = -2 outside the component.
 *   O4. s(seed) = +1 (the caller has oriented the seed).  Walking away from the seed, s(i) = -1 iff s(parent) dot3(n_i,
 *       n_parent) < 0, dot3 the library's uncontracted one (m3d_fp.hpp) on the normals AS GIVEN: a zero or NaN dot leaves i
 *       unflipped whatever its parent's sign.  out_normals = s(i) n_i -- negation only, no renormalisation; points with
 *       parent = -2 are returned unchanged.
 *   O5. stats: rounds = the Boruvka rounds run (the last one adds no edge unless the forest is complete before: at most
 *       ceil(log2 n) + 1), tree_edges = the edges of the whole forest, component = the size of the seed's component, flips.
 * radius must be finite and > 0, seed < n, n < 2^31; n == 0 is M3D_ERR_INVALID_ARG.  out_normals: n x 3, parent: n.
 * Results do not depend on what recycled device scratch holds. */
typedef struct m3d_orient_stats {
    uint64_t rounds, tree_edges, component, flips;
    double ms_total;  /* host clock, the whole call */
    double ms_grid;   /* upload + grid build (host clock around their wait) */
    double ms_rounds; /* the Boruvka rounds, edge list on the host included */
    double ms_signs;  /* the host's breadth-first pass */
} m3d_orient_stats;
int m3d_orient_normals_mst(const double *xyz, const double *normals, size_t n, double radius, size_t seed, int device,
                           double *out_normals, int64_t *parent, m3d_orient_stats *stats);

/* MODEL PREPARATION (m3d_ppf_prepare_model): a host composition on one device.
 *   B1. Box.  Mean and covariance of all points as Open3D's ComputeMeanAndCovariance: nine cumulants (x, y, z, xx, xy, xz,
 *       yy, yz, zz) summed serially in index order, divided by n, cov(a, b) = E[ab] - E[a] E[b].  Axes: the Jacobi sweeps of
 *       m3d_eig3.hpp.  extent_k = max - min of dot3(axis_k, p - mean); centre = mean + sum_k axis_k (max_k + min_k) / 2.
 *       With box_center and box_extent (3 doubles each, both or neither) they are used as given: a caller who has Open3D
 *       passes GetOrientedBoundingBox()'s and gets the reference's parameters.  The reference's box is the PCA box of Qhull's
 *       convex-hull vertices, which this build does not restate; only the extent and the centre are used, and both are
 *       invariant under the axes' order and signs.
 *   B2. diameter = sqrt(d0 d0 + d1 d1 + d2 d2); r_min = sqrt of the sum of the two smallest extents squared; dist_step =
 *       diameter rel_sample_dist; dist_step_dense = diameter rel_dense_sample_dist; normal_r = diameter calc_normal_relative;
 *       view_pt = centre + (0, 0, 2 diameter).
 *   B3. normals == NULL: m3d_estimate_normals(Hybrid, normal_r, 30, no orientation).  Then NormalizeNormals: s = (x x + y y) +
 *       z z, each component divided by sqrt(s) when s > 0.
 *   B4. seed = the point nearest view_pt (d2, lowest index at ties).  Unless normals were given and use_external_normal is
 *       set: the seed's normal is negated iff dot3(view_pt - p_seed, n_seed) < 0, once more if invert_model_normal, then
 *       O1 - O4 with radius = normal_r.
 *   B5. Sampler S(step), DownSamplePCNormal (:1018-1061) as written: a FIFO starts at the seed; pop cur, skip it if checked,
 *       else mark it checked and select it; its neighbours are the points with d2 < (2 step)^2 in ascending (d2, index); each
 *       one not checked is marked checked if sqrt(d2) < step, else pushed.  The result is the selection order.  Host.
 *   B6. sample = S(dist_step).  rel_dense_sample_dist > 0: dense = S(dist_step_dense) and edge_indices =
 *       m3d_detect_boundary_points(dense points, dense normals, Hybrid(normal_r, pts_num), 90 degrees), ascending, into dense.
 * out_normals: n x 3, the prepared normals of all points.  sample_indices / dense_indices / edge_indices: capacity n each;
 * dense_indices and edge_indices may be NULL when rel_dense_sample_dist <= 0.  n == 0: M3D_ERR_INVALID_ARG "There is no input
 * points"; a non-finite point is M3D_ERR_INVALID_ARG. */
typedef struct m3d_ppf_train_params {
    double rel_sample_dist;       /* 0.05 */
    double rel_dense_sample_dist; /* 0.025; <= 0: no dense sample, no edges (SampledPoints mode) */
    double calc_normal_relative;  /* 0.01 */
    int32_t invert_model_normal;  /* 0 */
    int32_t use_external_normal;  /* 0 */
    int32_t pts_num;              /* 20: edge_param_.pts_num */
    int32_t reserved;
} m3d_ppf_train_params;
void m3d_ppf_train_params_default_(m3d_ppf_train_params *p);
typedef struct m3d_ppf_model_info {
    double box_center[3], box_extent[3];
    double diameter, r_min, dist_step, dist_step_dense, normal_r, view_pt[3];
    uint64_t seed;          /* B4 */
    int32_t seed_flipped;   /* the seed's normal was negated in B4 */
    int32_t oriented;       /* O1 - O4 ran */
    m3d_orient_stats orient;
    uint64_t sample_distance_evaluations, dense_distance_evaluations;
    double ms_total, ms_box, ms_normals, ms_sample, ms_dense, ms_edges;
} m3d_ppf_model_info;
int m3d_ppf_prepare_model(const double *xyz, const double *normals, size_t n, const m3d_ppf_train_params *params,
                          const double *box_center, const double *box_extent, int device, double *out_normals,
                          size_t *sample_indices, size_t *n_sample, size_t *dense_indices, size_t *n_dense,
                          size_t *edge_indices, size_t *n_edges, m3d_ppf_model_info *info);
/* Estimate's reference points (:304-309): RandomSampler<size_t>(num).SampleWithoutDuplicate(sample) on std::mt19937(seed),
 * include/misc3d/utils.h:101-116 as written (its swap(indices[i], indices[rng() % num]) is not Fisher-Yates).  Host only.
 * out: `sample` entries; sample <= num < 2^32 (M3D_ERR_INVALID_ARG otherwise). */
int m3d_ppf_reference_indices(size_t num, size_t sample, uint32_t seed, size_t *out);

/* ---- PPF pose clustering: ClusterPoses, PoseAverage, RefineSparsePose, the centre shift and the scoring of
 * misc3d::pose_estimation::PPFEstimator, src/ppf_estimation.cpp -------------------------------------------------------------
 * Raw poses in, ranked and refined Pose6D results out: ClusterPoses (:871-935) with GatherPose (:778-836), CalcPoseNeighbor
 * (:838-869) and MatchPose (:745-776), PoseAverage (:992-1016), RefineSparsePose (:937-990), the centre shift (:342-351) and the
 * scoring (:353-392).  m3d_ppf_cluster_poses is K1 - K6, m3d_ppf_estimate is the vote and K1 - K8 (Estimate from :304 on).
 * PreprocessTrain is the block "PPF model preprocessing" above.  The text below is the contract; tests/cpp/ppf_cluster_ref.c restates it in serial C.
 *
 * INPUT.  poses[P] (row-major 4 x 4 doubles, poses of the CENTRED model as m3d_ppf_vote returns them) and votes[P].
 *   K1. Order: by votes descending, ties by ascending input index (the reference's std::sort leaves ties open; m3d_ppf_vote's
 *       output order is (reference position, model index), so this order is a fixed one).  Every index below is a position
 *       in this sorted list.
 *   K2. Cut: threshold = size_t(votes[0] 0.5); the valid poses are the prefix with votes >= threshold (:880-886).
 *   K3. Translation neighbours (:888-907): j is a neighbour of i (and i of itself) when d2 < r r, d2 = (dx dx + dy dy) + dz dz
 *       without contraction, r = dist_threshold (the reference's rel_dist_thresh_ x diameter), r r computed once on the host.
 *       d2 < r^2 is the library's neighbourhood rule and nanoflann's.
 *   K4. GatherPose, restated without its stack.  min_num_pt = int(max(6, the largest neighbour count) / 2.0).  A pose is a
 *       core when its count, itself included, is >= min_num_pt.  A cluster is a connected component of cores under the
 *       neighbour relation.  A non-core pose joins the cluster that starts first among the clusters of its core neighbours --
 *       a cluster starts at its lowest core index, so that is the cluster with the lowest minimum core index -- and is dropped
 *       when it has no core neighbour.  Cluster votes are the integer sum of member votes.  Clusters are sorted by votes
 *       descending, ties by lowest member.  Members are kept in ascending index.
 *   K5. Level 2, inside each translation cluster with its members ascending.  The match relation is MatchPose(.., 3)'s:
 *       d2 < r r and ca > cos_edge, ca = (trace - 1) / 2, trace the serial sum of the nine products src(r, c) dst(r, c) in
 *       row-major order, cos_edge = cos(angle_threshold) computed once on the host.  No acos runs on the device: acos(ca) <
 *       thr is ca > cos(thr), and the reference's clamps at ca > 1 and ca < -1 fall out of the compare.  Level 2 uses d2 < r r
 *       where the reference compares norm() < r; they differ only within an ulp of the threshold.  Then K4 again inside the
 *       cluster, with the cluster's own min_num_pt and the level-2 counts.
 *   K6. PoseAverage per sub-cluster, members ascending, on the host: the 10 distinct sums of q q^T with q = MatToQuat(R)
 *       (data_structure.h:58-87), the three t sums, the integer vote sum; the eigenvector of the largest eigenvalue by a
 *       cyclic Jacobi solver for the symmetric 4 x 4, signed so that its component of largest magnitude (lowest index on ties)
 *       is positive; t_avg = sum x (1.0 / count); the pose by QuatToMat.
 *   K7. Refinement per translation cluster that has at least one sub-cluster, in translation-cluster order: the averaged pose
 *       with the most votes (the first wins ties: std::max_element); ICP of the model's centred points against the scene from
 *       that pose, max_correspondence_distance = rel_dist_sparse_thresh x dist_step, criteria (1e-6, 1e-6, 30).
 *       refine_method: M3D_PPF_REFINE_NONE, M3D_PPF_REFINE_POINT_TO_POINT (the body of m3d_registration_icp) or
 *       M3D_PPF_REFINE_POINT_TO_PLANE (the body of m3d_registration_icp_plane_l1), unchanged, on the call's own lane.  The result
 *       keeps the picked sub-cluster's votes.
 *   K8. Centre shift T(i, 3) -= (c0 T(i, 0) + c1 T(i, 1)) + c2 T(i, 2); a STABLE sort by votes descending; expected =
 *       ((ratio n) n) 0.25 with n the model size (0.25 is VOTES_NUM_REDUCTION_FACTOR of the SampledPoints mode; an EdgePoints
 *       model: rule E9), score = min(1.0, votes / expected); results are cut at the first score below score_thresh and capped at
 *       num_result; q and t of each result by MatToQuat, as UpdateByPose does.
 * WHERE THE REFERENCE'S ORDER IS ARRIVAL ORDER.  The reference keeps a cluster's members in the depth-first order in which its
 * stack met them, and walks level 2 in that order; here members are ascending.  At level 1 the member sets are the reference's
 * exactly.  At level 2 the order decides only two things: which sub-cluster a border pose with core neighbours in two
 * sub-clusters joins, and the order of sub-clusters whose votes tie.  PoseAverage adds the members in depth-first order there,
 * so its floating-point sums can differ in the last bits.  RefineSparsePose appends its results inside a `critical` section:
 * here they come in translation-cluster order.
 * REFUSALS AND EMPTY CASES.  M3D_ERR_INVALID_ARG: a non-finite pose entry; dist_threshold not positive and finite;
 * angle_threshold outside (0, pi]; ratio, score_thresh or rel_dist_sparse_thresh not finite, or ratio <= 0; an unknown
 * refine_method.  M3D_OK with zero results: P == 0, or no clusters (the reference's `return false`).  More than 262 144 valid
 * poses (K2's prefix): M3D_ERR_CAPACITY.  The call's device scratch is 124 bytes a valid pose, 31 MiB at that cap.
 * DEVICE ("PPF pose clustering").  Per level six launches on one lane and one stream: a tiled all-pairs count
 * (256 poses a workgroup, the j side through LDS in tiles of 256), an atomic max (one word at level 1, one per translation
 * cluster at level 2 -- the host makes no round trip between the launches or the levels), the core flags, a lock-free union of
 * matching cores that hooks the larger root under the smaller, a flatten pass, and the border poses' minimum root.  Every
 * output of the device is an integer (counts, flags, labels) and none depends on scheduling or on how the j range is split
 * over workgroups.  One read-back carries counts, labels and largest counts of both levels; K1, K2 and K6 - K8 are the host's. */
#define M3D_PPF_REFINE_NONE 0
#define M3D_PPF_REFINE_POINT_TO_POINT 1
#define M3D_PPF_REFINE_POINT_TO_PLANE 2
typedef struct m3d_ppf_cluster_params {
    double dist_threshold;          /* rel_dist_thresh_ x diameter: 0.05 x diameter */
    double angle_threshold;         /* rel_angle_thresh_ in RADIANS (12 degrees = pi / 15) */
    double ratio;                   /* ref_param_.ratio, 0.6 */
    double score_thresh;            /* score_thresh_, 0.6 */
    double rel_dist_sparse_thresh;  /* refine_param_.rel_dist_sparse_thresh, 5 */
    int32_t num_result;             /* num_result_, 10 */
    int32_t refine_method;          /* M3D_PPF_REFINE_*, PointToPlane */
    int32_t object_id;              /* object_id_, 0: copied to the results by the callers' wrappers */
    int32_t reserved;
} m3d_ppf_cluster_params;
typedef struct m3d_ppf_cluster_stats {
    uint64_t n_valid;      /* poses that survive K2 */
    uint64_t clusters_t;   /* translation clusters (level 1) */
    uint64_t clusters_r;   /* sub-clusters of all translation clusters (level 2) = averaged poses */
    uint64_t pair_tests;   /* 6 n_valid^2: three all-pairs launches a level */
    uint32_t launches;     /* kernel launches of the clustering */
    uint32_t splits;       /* workgroups that share the j tiles of a row block */
    double ms_device;      /* HIP events around the clustering's device work */
    double ms_total;       /* wall clock of the call */
} m3d_ppf_cluster_stats;
typedef struct m3d_ppf_estimate_stats {
    m3d_ppf_vote_stats vote;
    m3d_ppf_cluster_stats cluster;
    uint64_t n_raw;        /* raw poses of the vote */
    uint32_t icp_calls;    /* K7's ICP calls */
    uint32_t icp_iterations;
    double ms_vote, ms_cluster, ms_refine, ms_host;   /* wall clock: the vote, K1 - K6, K7, and the rest (K8, copies) */
    double ms_total;
} m3d_ppf_estimate_stats;
/* the reference's defaults; dist_threshold = 0.05 x the model's diameter (model == NULL: 0.05) */
void m3d_ppf_default_cluster_params(const m3d_ppf_model *model, m3d_ppf_cluster_params *out);
/* K1 - K6.  Per valid pose (pose_capacity entries each): order (its input index), count_t / count_r (neighbour counts of the
 * two levels, count_r 0 outside every translation cluster), label_t (the rank of its translation cluster, -1: dropped),
 * label_r (the rank of its sub-cluster inside that cluster, -1: dropped).  min_num_pt_t: one value.  Per translation
 * cluster (cluster_capacity entries each): min_num_pt_r, cluster_votes.  Per averaged pose, in (translation cluster,
 * sub-cluster) order (cluster_capacity entries each): avg_poses (x 16 doubles), avg_votes, avg_cluster (its translation
 * cluster).  *n_valid, *n_clusters_t and *n_clusters_r are always set.  n_valid > pose_capacity, or a cluster count >
 * cluster_capacity: M3D_ERR_CAPACITY, nothing is written to the arrays, and the three counts say what the call needs.  Every
 * array may be NULL when its capacity is 0. */
int m3d_ppf_cluster_poses(const double *poses, const uint32_t *votes, size_t P, const m3d_ppf_cluster_params *params, int device,
                          size_t pose_capacity, size_t *n_valid, uint32_t *order, uint32_t *count_t, int32_t *label_t,
                          uint32_t *count_r, int32_t *label_r, size_t cluster_capacity, size_t *n_clusters_t, size_t *n_clusters_r,
                          int32_t *min_num_pt_t, int32_t *min_num_pt_r, uint64_t *cluster_votes, double *avg_poses,
                          uint64_t *avg_votes, uint32_t *avg_cluster, m3d_ppf_cluster_stats *stats);
/* The vote and K1 - K8.  scene_points / scene_normals / reference as m3d_ppf_vote takes them; params == NULL: the defaults.
 * Results (capacity entries each; capacity >= num_result always suffices): poses (x 16 doubles, of the UNCENTRED model), q (x 4:
 * w, x, y, z), t (x 3), votes, scores.  More results than capacity: M3D_ERR_CAPACITY with *n_results the needed count. */
int m3d_ppf_estimate(const m3d_ppf_model *model, const double *scene_points, const double *scene_normals, size_t m,
                     const size_t *reference, size_t n_ref, const m3d_ppf_cluster_params *params, size_t capacity,
                     size_t *n_results, double *poses, double *q, double *t, uint64_t *votes, double *scores,
                     m3d_ppf_estimate_stats *stats);
/* The same for an EdgePoints model (rule E9 of "PPF voting, EdgePoints mode"): the vote of m3d_ppf_vote_edges, K1 - K7 with the
 * ICP against the scene SAMPLE, K8 with expected = (ratio n) n.  Results and stats as m3d_ppf_estimate. */
int m3d_ppf_estimate_edges(const m3d_ppf_model *model, const double *scene_points, const double *scene_normals, size_t m,
                           const size_t *reference, size_t n_ref, const double *scene_edge_points,
                           const double *scene_edge_normals, size_t m_edge, const m3d_ppf_cluster_params *params,
                           size_t capacity, size_t *n_results, double *poses, double *q, double *t, uint64_t *votes,
                           double *scores, m3d_ppf_estimate_stats *stats);

/* ---- misc -------------------------------------------------------------------------------------- */
const char *m3d_last_error(void); /* thread-local; reference message text for M3D_ERR_* */
int m3d_device_count(void);       /* 0 when no HIP device is usable */
const char *m3d_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MISC3D_AMD_H */
