"""Run every BASELINE.json configuration once at full size on ONE MI355X and print a JSON line per
config (timings from the C ABI's own clocks + wall clock).  Not the headline bench (that is
bench.py); these lines feed DESIGN.md section 6 and check that the full sizes run at all.

  C1 fit_plane 50k pts, 100 iters (plumbing)            C2 fit_plane 1M pts, 10k hyp (= bench.py)
  C3 fit_cylinder + fit_sphere 1M pts, 50k hyp          C4 match + compute_transformation_ransac 200k<->200k, 100k hyp
  C5 segment_plane_iterative 10M pts (single GPU leg)
  P1 / P2 farthest_point_sampling 5 841 x 1 000 (the reference example) / 1M x 10 000, every device path (A/B)
  S1 - S4 ProximityExtractor.segment: the reference example's shape, the raw golden PLY at r = 0.01, 1 M and 10 M synthetic
  K1 - K4 KNearestSearch: 200k x 200k x 33 k=10 batched, 1 000 single-query calls, 1 M x 3 k=30 (grid, tile A/B),
          50k x 33 k=1000 (select)
  V1 - V3 voxel_down_sample: the 1 M-point bench scene at 0.005 / 0.02 of its extent, and the three-level call
  I1 registration_icp_plane against registration_icp at the C4 ICP shape (200k x 200k, 0.02), alternating in one process
  I2 refine_fragment_pair ({v, v/2, v/4}, {50, 30, 15}) on 50 000-point fragments, with its per-level split (point-to-plane,
     point-to-point and coloured)
  R1 - R3 RayCastRenderer: the reference example (640 x 480, obj.ply at its two poses), 1920 x 1080 with 64 instances, and a
          100-frame batch of the example
  PV1 PPFVoting: the table of a 2 000-point model and the vote of a 20 000-point scene at ratio 0.6, LDS / device memory A/B
  PC1 PPF pose clustering on PV1's scene: the vote's raw poses through m3d_ppf_cluster_poses, and the whole m3d_ppf_estimate
  PV2 PPFVoting in EdgePoints mode at PV1's sizes: a plate with holes, its edge sets by detect_boundary_points; table, vote, estimate
  PT1 PPF model preprocessing (PreprocessTrain) and PPFEstimator.train on a synthetic closed surface of 1 M and of 100 k points,
      default config: the orientation's Boruvka rounds against the restatement's heap walk, the host samplers, boundary detection
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from misc3d_amd import capi, synth  # noqa: E402

NO_CPU = "--no-cpu-baseline" in sys.argv or bool(os.environ.get("M3D_NO_CPU_BASELINE"))   # (runs under the profiler)
_args = [a for a in sys.argv[1:] if not a.startswith("--")]
which = set(_args) or {"C1", "C2", "C3", "C4", "C5"}
ALL = len(_args) == 0
sys.path.insert(0, os.path.join(ROOT, "tools"))


def cpu(fn, *a, **kw):
    """the cpu_baseline object of a line (tools/cpu_baselines.py: the oracle's restatement of the reference's CPU path on this
    box's cores, a bounded sample), or None under --no-cpu-baseline"""
    if NO_CPU:
        return None
    import cpu_baselines
    return getattr(cpu_baselines, fn)(*a, **kw)

HBM_PEAK_GBS = 8000.0
FP64_VALU_PEAK_TOPS = 39.3      # 256 CU x 4 SIMD x 16 fp64 lanes/clk x 2.4 GHz, non-FMA ops (bench.py)
MFMA_F16_PEAK_TFLOPS = 2500.0   # dense fp16 MFMA (MI355X_MICROARCH.md)
N4_COUNTS = (55576.0, 18203.0)   # boundary_k: (VALU, LDS) instructions per wave of 64 points (one point per lane) -- from profiles/r06_pmc_boundary.txt
VALU_OPS_FP64 = {0: 7, 1: 10, 2: 22}    # score_mask_k: fp64 VALU instructions per (point, hypothesis)
VALU_OPS_SCREEN = {0: 3.625, 1: 4.125, 2: 6.125}   # score_screen_k: packed-fp32 screen, 29 / 33 / 49 instructions per 8 points; bench.py has the count
capi.set_config(kernel_timing=1)  # the fit rooflines need m3d_stats.ms_score_kernel (HIP events around the scoring launches)


def fit_roofline(kind, st):
    """VALU-issue roofline of the scoring launches of ONE fit, from the library's own counters: (tile, hypothesis)
    pairs evaluated x 512 points x VALU instructions per (point, hypothesis) / time of the scoring launches (HIP events).
    Recomputable from profiles/r02_configs_kernel_stats.csv (same launches, AverageNs x Calls of score_screen_k<kind> /
    score_mask_k<2>)."""
    if not st["ms_score_kernel"]:
        return None
    screened = bool(capi.get_config().score_fp32_screen)
    ops = (VALU_OPS_SCREEN if screened else VALU_OPS_FP64)[kind]
    tops = st["pairs_timed"] * 512.0 * ops / (st["ms_score_kernel"] * 1e-3) / 1e12   # (pairs of the timed launches: m3d_stats.pairs_timed)
    # the peak priced per instruction class (bench.py: CLASS_CYCLES from tools/ubench/valu_rates.hip, the loops' instruction mixes)
    import bench as _b
    n_mix, cyc_mix, _ = _b.peak_model((_b.MIX_SCREEN if screened else _b.MIX_FP64)[kind])
    peak = _b.SIMDS * 64.0 * _b.CLOCK_HZ / (cyc_mix / n_mix) / 1e12
    frac = st["pairs_timed"] * cyc_mix / (st["ms_score_kernel"] * 1e-3 * _b.SIMDS * _b.CLOCK_HZ)
    return {"bound": "valu-issue", "kernel": f"m3d::score_{'screen' if screened else 'mask'}_k<{kind}>", "achieved": tops,
            "peak": peak, "unit": "T lane-instructions/s (VALU issue)", "frac": frac,
            "frac_if_every_instruction_took_4_cycles": tops / FP64_VALU_PEAK_TOPS,
            "ops_per_pair": ops, "pairs_recounted_in_fp64": st["pairs_exact"],
            "launches": st["score_launches"], "kernel_ms_total": st["ms_score_kernel"], "tile_hypothesis_pairs": st["pairs_timed"], "pairs_of_the_untimed_lead_pass": st["pairs_scored"] - st["pairs_timed"]}


def emit(name, **kw):
    print(json.dumps({"config": name, **kw}), flush=True)


def timed_fit(cloud, kind, thr, H, prob, seed, reps=3):
    """(seconds, Fit) of the fastest of `reps` x 5 fits after enough of them to bring the clocks up (>= 40 ms of fits: a cold
    GPU times its first fits 5-8 % long, bench.py PRIMING_FITS); Fit.stats["ms_plain"] = the same with m3d_config.kernel_timing =
    0, the library's default (no HIP events attached to the scoring launches)."""
    t_end = time.perf_counter() + 0.04
    cloud.fit(kind, thr, H, prob, seed=seed, copy=False)
    while time.perf_counter() < t_end:
        cloud.fit(kind, thr, H, prob, seed=seed, copy=False)
    best = None
    for _ in range(reps * 5):
        t0 = time.perf_counter()
        g = cloud.fit(kind, thr, H, prob, seed=seed, copy=False)
        dt = time.perf_counter() - t0
        if best is None or dt < best[0]:
            best = (dt, g)
    capi.set_config(kernel_timing=0)
    plain = None
    for _ in range(reps * 5):
        t0 = time.perf_counter()
        cloud.fit(kind, thr, H, prob, seed=seed, copy=False)
        dt = time.perf_counter() - t0
        plain = dt if plain is None else min(plain, dt)
    capi.set_config(kernel_timing=1)
    best[1].stats["ms_plain"] = plain * 1e3
    return best


if "C1" in which:
    pts = synth.plane_cloud_c1(50_000, 1)
    with capi.Cloud(pts) as c:
        dt, g = timed_fit(c, 0, 0.01, 100, 0.9999, 7)
    emit("C1 fit_plane 50k x 100 iters p=0.9999", ms=dt * 1e3, iterations=g.stats["iterations"],
         n_inliers=g.stats["n_inliers"], params=g.params.tolist(), roofline=fit_roofline(0, g.stats),
         cpu_baseline=cpu("fit_baseline", 0, pts, None, 0.01, 7, 100, 2.0, "C1 fit_plane"))

if "C2" in which:
    pts = synth.plane_cloud_c2(1_000_000, 2)
    with capi.Cloud(pts) as c:
        dt, g = timed_fit(c, 0, 0.01, 10_000, 1.0, 11)
    emit("C2 fit_plane 1M x 10k hyp", ms=dt * 1e3, hyp_per_s=10_000 / dt, n_inliers=g.stats["n_inliers"],
         best_index=g.stats["best_index"], ms_without_timing_events=g.stats["ms_plain"],
         stats={k: g.stats[k] for k in ("ms_sample", "ms_score", "ms_refine")},
         roofline=fit_roofline(0, g.stats), cpu_baseline=cpu("fit_baseline", 0, pts, None, 0.01, 11, 10_000, 5.0, "C2 fit_plane"))

if "C3" in which:
    cp, cn = synth.cylinder_cloud_c3(1_000_000, 3)
    with capi.Cloud(cp, cn) as c:
        dt, g = timed_fit(c, 2, 0.01, 50_000, 1.0, 13, reps=2)
    emit("C3 fit_cylinder 1M x 50k hyp", ms=dt * 1e3, hyp_per_s=50_000 / dt, n_inliers=g.stats["n_inliers"],
         best_index=g.stats["best_index"], params=g.params.tolist(),
         ms_without_timing_events=g.stats["ms_plain"],
         stats={k: g.stats[k] for k in ("ms_sample", "ms_score", "ms_refine", "exact_rmse_evals")},
         roofline=fit_roofline(2, g.stats), cpu_baseline=cpu("fit_baseline", 2, cp, cn, 0.01, 13, 50_000, 6.0, "C3 fit_cylinder"))
    sp = synth.sphere_cloud_c3(1_000_000, 4)
    with capi.Cloud(sp) as c:
        dt, g = timed_fit(c, 1, 0.01, 50_000, 1.0, 13, reps=2)
    emit("C3 fit_sphere 1M x 50k hyp", ms=dt * 1e3, hyp_per_s=50_000 / dt, n_inliers=g.stats["n_inliers"],
         best_index=g.stats["best_index"], params=g.params.tolist(),
         ms_without_timing_events=g.stats["ms_plain"],
         stats={k: g.stats[k] for k in ("ms_sample", "ms_score", "ms_refine", "exact_rmse_evals")},
         roofline=fit_roofline(1, g.stats), cpu_baseline=cpu("fit_baseline", 1, sp, None, 0.01, 13, 50_000, 6.0, "C3 fit_sphere"))

if "C4" in which:
    n = int(os.environ.get("M3D_C4_POINTS", "200000"))
    d = synth.registration_pair_c4(n, seed=5)
    def timed_match():
        t0 = time.perf_counter()
        r = capi.match_mutual_nn(d["feat_src"], d["feat_dst"])
        return time.perf_counter() - t0, r
    t_match, (i0, i1) = timed_match()
    ts = sorted(timed_match()[0] for _ in range(7))     # (calls two to four of a process still get faster: pools, clocks)
    t_match2 = ts[len(ts) // 2]
    sliced = bool(capi.match_last_path() & 2)
    old_cfg = capi.set_config(match_pipeline=0)
    try:
        tw = sorted(timed_match()[0] for _ in range(5))
    finally:
        capi.restore_config(old_cfg)
    inv = np.empty(n, dtype=np.int64)
    inv[d["perm"]] = np.arange(n)
    true_frac = float(np.mean(inv[i0.astype(np.int64)] == i1.astype(np.int64)))
    # the screen is ONE fp16 contraction over all (query, row) pairs -- since round 3 a single scan serves both search directions,
    # since round 4 over the hi halves only (K = 48: 33 values, the norms' pieces, padding) -- plus the two warm-up passes (1/16
    # and 1/8 of it): n x n x 48 x 2 x (1 + 3/16) flop.  Priced with the WHOLE call's wall clock (106 MB of descriptors over
    # PCIe, packing, binning, the fp64 verifications): a lower bound of the kernel's own fraction.  pair_dist_per_s counts both
    # directions' distances.
    mm_flop = float(n) * n * 48 * 2 * (1.0 + 3.0 / 16.0)
    emit("C4 match_correspondence", n=n, dim=33, ms_first=t_match * 1e3, ms=t_match2 * 1e3, ms_best=ts[0] * 1e3,
         uploads_sliced_under_the_scan=sliced, ms_both_matrices_uploaded_first=tw[len(tw) // 2] * 1e3, matches=len(i0),
         true_fraction=true_frac, pair_dist_per_s=2.0 * n * n / t_match2,
         roofline={"bound": "mfma", "kernel": "m3d::nn16_scan_k<false, true> (one scan, both directions)",
                   "achieved": mm_flop / t_match2 / 1e12,
                   "peak": MFMA_F16_PEAK_TFLOPS, "unit": "TFLOP/s (fp16 MFMA, whole call's wall clock)",
                   "frac": mm_flop / t_match2 / 1e12 / MFMA_F16_PEAK_TFLOPS, "flop": mm_flop,
                   "note": "K = 48 since round 4 (hi halves only; K = 112 before): 3/7 of the flop per pair, so the fraction on the "
                           "smaller count is lower although the call is faster.  The scan ALONE, in one launch (profiles/r06_match_scan_findings.txt): "
                                   "3.8 ms = 0.40 of the peak on the nominal 3.84 TFLOP; matrix pipe busy 0.535 of the SIMD cycles, the VALU port "
                                   "nearly full at that rate (DESIGN 4)"},
         cpu_baseline=cpu("match_baseline", d["feat_src"], d["feat_dst"], 6.0))
    dts = []
    for _ in range(2):      # (the first call of a process also sizes the device's block free list: ~10 ms)
        t0 = time.perf_counter()
        T, st = capi.registration_ransac(d["src"], d["dst"], i0, i1, threshold=0.03, max_iter=100_000,
                                         edge_length_threshold=0.9, confidence=1.0, seed=17)
        dts.append(time.perf_counter() - t0)
    dt = dts[1]
    # every validation = one exact nearest-neighbour query per source point.  SURVEY.md 8(d)'s unit is 24 B per (hypothesis,
    # point); the kernel is bound by the L1's tag look-ups (a list-entry gather touches ~29 cache lines per instruction:
    # ~0.9 look-ups per cycle and CU) with VALU issue at ~60 % behind it, not by HBM (TA / TCP / SQ
    # counters of reg_validate_k: profiles/r02_pmc_reg_validate.txt)
    queries = float(st["validations"]) * n
    emit("C4 compute_transformation_ransac 200k<->200k x 100k hyp", ms=dt * 1e3, ms_first=dts[0] * 1e3, hyp_per_s=100_000 / dt,
         validations=st["validations"], fitness=st["fitness"], best_index=st["best_index"],
         pose_err=float(np.abs(T - d["T"]).max()),
         nn_fp32_screen=st["nn_fp32_screen"], nn_screen_fallbacks=st["nn_screen_fallbacks"],
         candidate_cache={"pairs_exact": st["lds_wave_hypotheses"], "pairs_left_as_bounds": st["global_wave_hypotheses"],
                          "note": "(256-point tile, hypothesis) pairs of the validation: every query answered from registers under a "
                                  "certificate / an upper bound of the count and a lower bound of the sum for the pruning, walked only if "
                                  "the hypothesis survives it (m3d_reg_cache.hip)"},
         roofline={"bound": "hbm (algorithmic unit of SURVEY 8(d): 24 B per (hypothesis, point) query); the kernels' own limits are VALU "
                            "issue (reg_validate_cached_k: ~315 instructions per 64 queries, no memory access) and the L1's gather rate "
                            "(reg_validate_pairs_k: the walk of the far poses)",
                   "kernel": "m3d::reg_validate_cached_k + m3d::reg_validate_pairs_k<true>", "achieved": queries * 24.0 / dt / 1e9,
                   "peak": HBM_PEAK_GBS, "unit": "GB/s",
                   "frac": queries * 24.0 / dt / 1e9 / HBM_PEAK_GBS, "queries": queries, "queries_per_s": queries / dt,
                   "note": "whole call's wall clock (setup, grid, 173 MB of neighbour lists, cache builds, replay included); queries = "
                           "validations x source points, the nominal unit -- the pruning phases evaluate ~73 % of them"},
         cpu_baseline=cpu("validation_baseline", d["src"], d["dst"], d["T"], 0.03, 6.0))
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        T2, st2 = capi.registration_ransac(d["src"], d["dst"], i0, i1, threshold=0.03, max_iter=100_000,
                                           edge_length_threshold=0.9, confidence=0.999, seed=17)
        ts.append((time.perf_counter() - t0) * 1e3)
    q2 = float(st2["validations"]) * n
    emit("C4 same with the reference's confidence 0.999", ms=sorted(ts)[1], ms_first=ts[0],
         iterations=st2["iterations"], validations=st2["validations"], pose_err=float(np.abs(T2 - d["T"]).max()),
         roofline={"bound": "latency: a handful of validations (the loop ends after ~24 iterations), each a dependent chain of short launches "
                            "and host round trips; on the 8(d) unit", "kernel": "m3d::reg_validate_k<false>",
                   "achieved": q2 * 24.0 / (sorted(ts)[1] * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                   "frac": q2 * 24.0 / (sorted(ts)[1] * 1e-3) / 1e9 / HBM_PEAK_GBS, "queries": q2},
         cpu_baseline={"see": "the line above: the same kd-tree validation, ms_per_validation x validations + the sequential loop"})
    # the step the reference's examples chain next: point-to-point ICP on the RANSAC pose (max distance 0.02)
    ts = []
    for _ in range(3):      # one-call entry point: median of three (the first call also warms the block free list)
        t0 = time.perf_counter()
        T3, st3 = capi.registration_icp(d["src"], d["dst"], 0.02, T2)
        ts.append((time.perf_counter() - t0) * 1e3)
    q3 = float(st3["iterations"]) * n

    def icp_cpu():
        import oracle
        t0 = time.perf_counter()
        m = 4000      # (brute-force correspondences: a slice of the source)
        oracle.registration_icp(d["src"][:m], d["dst"], 0.02, T2, max_iter=3)
        dt_c = time.perf_counter() - t0
        return {"value": 3 * m / dt_c, "unit": "correspondence queries/s", "cores": oracle.usable_cpus(), "kind": "port",
                "sample": f"3 ICP iterations of the first {m} source points against all {n} target points, brute-force nearest neighbour "
                          f"(OpenMP), {dt_c:.1f} s", "flags": "-O3 -ffp-contract=off (no -march)"}
    emit("C4 registration_icp on that pose (point-to-point, 0.02, 30 it)", ms=sorted(ts)[1], ms_first=ts[0],
         iterations=st3["iterations"], fitness=st3["fitness"], rmse=st3["inlier_rmse"],
         pose_err=float(np.abs(T3 - d["T"]).max()),
         roofline={"bound": "hbm on the 8(d) unit (24 B per query); the call is a chain of short launches per iteration (grid search, sums, "
                            "3x3 solve on the host)", "kernel": "m3d::icp_nn_k + umeyama_sums_k<PASS, IcpPairs>", "achieved": q3 * 24.0 / (sorted(ts)[1] * 1e-3) / 1e9,
                   "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": q3 * 24.0 / (sorted(ts)[1] * 1e-3) / 1e9 / HBM_PEAK_GBS, "queries": q3},
         cpu_baseline=None if NO_CPU else icp_cpu())

if "N2" in which or ALL:
    # ReconstructionPipeline::GlobalRegistration over many fragment pairs (src/pipeline.cpp:428-439: one
    # std::thread per pair) -- m3d_global_registration_batch on ONE device with 1 / 2 / 4 / 8 pairs in flight (lanes).  Fragments
    # of M3D_N2_POINTS points (default 50 000: a 3 m fragment at 1.4 cm voxels), 33-D descriptors, 12 fragments' worth of pairs
    # drawn from 6 distinct synthetic pairs, the reference's defaults (max_iter 100 000, confidence 0.999).
    nfrag = int(os.environ.get("M3D_N2_POINTS", "50000"))
    base = [synth.registration_pair_c4(nfrag, seed=50 + k) for k in range(6)]
    pairs = [(b["src"], b["dst"], b["feat_src"], b["feat_dst"]) for b in base] * 4       # 24 pairs
    seeds = [1000 + k for k in range(len(pairs))]
    vox = 0.03 / 1.4
    capi.global_registration_batch(pairs[:4], vox, seeds=seeds[:4], inflight=1)            # warm the lanes' pools
    old_lanes = capi.set_config(lanes=8)
    ref = None
    rows = {}
    for inflight in (1, 2, 4, 8):
        capi.global_registration_batch(pairs[:inflight * 2], vox, seeds=seeds[:inflight * 2], inflight=inflight)   # warm every lane
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            res = capi.global_registration_batch(pairs, vox, seeds=seeds, inflight=inflight, want_stats=True)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        if ref is None:
            ref = res
        same = all(a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(ref, res))
        rows[inflight] = {"ms": best * 1e3, "pairs_per_s": len(pairs) / best, "identical_to_serial": bool(same),
                          "lanes_used": len({r[3]["lane"] for r in res})}
    # the same 24 pairs as the reference holds them: 12 fragments resident for the call, pairs by index
    frs = [b["src"] for b in base] + [b["dst"] for b in base]
    fes = [b["feat_src"] for b in base] + [b["feat_dst"] for b in base]
    ipairs = [(k, 6 + k) for k in range(6)] * 4
    resident = {}
    for inflight in (1, 4, 8):
        capi.register_fragment_pairs(frs, fes, ipairs[:inflight * 2], vox, seeds=seeds[:inflight * 2], inflight=inflight)
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            res = capi.register_fragment_pairs(frs, fes, ipairs, vox, seeds=seeds, inflight=inflight, want_stats=True)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        same = all(a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(ref, res))
        resident[inflight] = {"ms": best * 1e3, "pairs_per_s": len(ipairs) / best, "identical_to_serial": bool(same)}
        if inflight == 1:   # a pair alone on resident fragments (the later ones of the call: their fragments are there already)
            late = [r[3] for r in res[12:]]
            resident[inflight]["per_pair_ms"] = {k: float(np.median([st[k] for st in late])) for k in ("ms_match", "ms_ransac", "ms_info", "ms_total")}
    capi.restore_config(old_lanes)
    st = {k: float(np.median([r[3][k] for r in ref])) if k != "n_matches" else ref[0][3][k] for k in ("ms_match", "ms_ransac", "ms_info", "ms_total", "n_matches")}
    def n2_cpu():
        import oracle
        m = 8000      # (brute-force matcher: a capped fragment)
        b0 = synth.registration_pair_c4(m, seed=50)
        oracle.set_omp_threads(oracle.usable_cpus())
        t0 = time.perf_counter()
        oracle.global_registration(b0["src"], b0["dst"], b0["feat_src"], b0["feat_dst"], vox, seed=1000)
        dt_c = time.perf_counter() - t0
        return {"value": 1.0 / dt_c, "unit": f"pairs/s at {m} points per fragment", "cores": oracle.usable_cpus(), "kind": "port",
                "sample": f"one pair of {m}-point fragments (the GPU's have {nfrag}: the matcher's work goes with the square), {dt_c:.1f} s: "
                          "brute-force mutual NN (OpenMP) + the sequential RANSAC loop + the information matrix",
                "flags": "-O3 -ffp-contract=off (no -march)"}
    emit(f"N2 global_registration_batch {len(pairs)} pairs of {nfrag} pts x 33-D, one device", accepted=int(sum(r[0] for r in ref)),
         per_pair_serial_ms={k: st[k] for k in ("ms_match", "ms_ransac", "ms_info", "ms_total")}, matches=st["n_matches"],
         in_flight=rows, speedup_over_serial={k: rows[1]["ms"] / v["ms"] for k, v in rows.items()},
         fragments_resident=resident, resident_speedup_over_serial_batch={k: rows[1]["ms"] / v["ms"] for k, v in resident.items()},
         note="pairs are independent (no collective); what overlaps is one pair's uploads and host-side steps (cross-check, "
              "RANSAC replay, grid set-up) with another pair's kernels",
         roofline={"bound": "mfma (the matcher is 2/3 of a pair) on the fp16 screen's flop", "kernel": "m3d::nn16_scan_k (per pair) + the pair's "
                            "registration", "achieved": 2.0 * nfrag * nfrag * 48 * (1 + 3.0 / 16.0) * rows[4]["pairs_per_s"] / 1e12,
                   "peak": MFMA_F16_PEAK_TFLOPS, "unit": "TFLOP/s (fp16 MFMA, 4 pairs in flight)",
                   "frac": 2.0 * nfrag * nfrag * 48 * (1 + 3.0 / 16.0) * rows[4]["pairs_per_s"] / 1e12 / MFMA_F16_PEAK_TFLOPS},
         cpu_baseline=None if NO_CPU else n2_cpu())

if "LANES" in which or ALL:
    # lanes (m3d_driver.hpp): independent callers on ONE device -- T host threads, each with its own resident 200 000-point cloud,
    # each running fit_plane(thr 0.01, 1000 iterations, probability 0.9999) in a loop, and the same with the one-shot m3d_fit_plane
    # from host arrays (upload + fit + list back per call); fits per second of all threads together.
    import threading
    npts = 200_000
    clouds_xyz = [synth.plane_cloud_c1(npts, 100 + t) for t in range(8)]
    old_cfg = capi.set_config(lanes=8, kernel_timing=0)
    rows = {}
    for mode in ("resident", "one_shot"):
        rows[mode] = {}
        for T in (1, 2, 4, 8):
            clouds = [capi.Cloud(clouds_xyz[t]) for t in range(T)] if mode == "resident" else None
            reps = 300 if mode == "resident" else 100
            start = threading.Barrier(T + 1)

            def work(t):
                f = (lambda: clouds[t].fit(0, 0.01, 1000, 0.9999, seed=7, copy=False)) if mode == "resident" else \
                    (lambda: capi.fit(0, clouds_xyz[t], None, 0.01, 1000, 0.9999, seed=7, copy=False))
                for _ in range(10):
                    f()
                start.wait()
                for _ in range(reps):
                    f()
                start.wait()

            ths = [threading.Thread(target=work, args=(t,)) for t in range(T)]
            for th in ths:
                th.start()
            start.wait()
            t0 = time.perf_counter()
            start.wait()
            dt = time.perf_counter() - t0
            for th in ths:
                th.join()
            rows[mode][T] = {"fits_per_s": T * reps / dt, "ms_per_fit_per_thread": dt / reps * 1e3}
            if clouds:
                for c in clouds:
                    c.close()
    # ... and the same fits handed over as ONE call from ONE python thread: m3d_cloud_fit_batch, the clouds on lanes of their own
    # (m3d_cloud_create_lane) -- the loop runs on threads of the library, the interpreter's lock is released once
    rows["batch"] = {}
    for T in (1, 2, 4, 8):
        clouds = [capi.Cloud(clouds_xyz[t], lane=t) for t in range(T)]
        per = 200
        jobs = [(clouds[t], 0, 0.01, 1000, 0.9999, 7) for _ in range(per) for t in range(T)]
        capi.fit_batch(jobs[: 10 * T], want_inliers=False)
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            res = capi.fit_batch(jobs, want_inliers=False)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        rows["batch"][T] = {"fits_per_s": len(jobs) / best, "ms_per_fit_per_lane": best / per * 1e3}
        for c in clouds:
            c.close()
    capi.restore_config(old_cfg)
    capi.set_config(kernel_timing=1)
    def lanes_cpu():
        import oracle
        oracle.set_omp_threads(oracle.usable_cpus())
        t0 = time.perf_counter()
        reps_c = 5
        for _ in range(reps_c):
            oc = oracle.fit(0, clouds_xyz[0], None, thr=0.01, max_iter=1000, prob=0.9999, seed=7, lookahead=8 * oracle.usable_cpus())
        dt_c = (time.perf_counter() - t0) / reps_c
        return {"value": 1.0 / dt_c, "unit": "fits/s", "cores": oracle.usable_cpus(), "kind": "port",
                "sample": f"the same fit ({npts} points, adaptive stop after {oc.iterations} iterations), {reps_c} times, the records of the next "
                          "hypotheses computed ahead by an OpenMP team", "flags": "-O3 -ffp-contract=off (no -march)"}
    emit(f"LANES fit_plane {npts} pts x 1000 iterations (adaptive stop), T threads on one device", **rows,
         speedup={m: {T: rows[m][T]["fits_per_s"] / rows[m][1]["fits_per_s"] for T in rows[m]} for m in rows},
         roofline={"bound": "latency: a fit of a few dozen hypotheses is a chain of ~8 short launches and one host wait (~80 us); on the "
                            "8(d) unit (24 B x points per scored hypothesis) it is far from any bandwidth",
                   "kernel": "the whole fit", "achieved": rows["resident"][4]["fits_per_s"] * npts * 24.0 * 38 / 1e9, "peak": HBM_PEAK_GBS,
                   "unit": "GB/s (38 hypotheses per fit, 4 threads)", "frac": rows["resident"][4]["fits_per_s"] * npts * 24.0 * 38 / 1e9 / HBM_PEAK_GBS},
         cpu_baseline=None if NO_CPU else lanes_cpu())

if "N3" in which or ALL:
    # EstimateNormalsFromMap at the reference example's size (848 x 480, k = 3) and at 4 Mpixel
    def n3_cpu(xyz, w, h, k):
        import oracle
        t0 = time.perf_counter()
        oracle.normals_from_map(xyz, w, h, k)
        dt_c = time.perf_counter() - t0
        return {"value": w * h / dt_c / 1e6, "unit": "Mpixel/s", "cores": 1, "kind": "port",
                "sample": f"the whole {w} x {h} map once, {dt_c * 1e3:.0f} ms (src/normal_estimation.cpp:64-207 is a serial loop)",
                "flags": "-O3 -ffp-contract=off (no -march)"}
    for (w, h, k) in ((848, 480, 3), (2048, 2048, 5)):
        rng = np.random.default_rng(1)
        u, v = np.meshgrid(np.arange(w), np.arange(h))
        z = 1.0 + 0.001 * u + 0.002 * v + rng.normal(0, 1e-4, (h, w))
        xyz = np.stack([(u - w / 2) / 500.0 * z, (v - h / 2) / 500.0 * z, z], -1).reshape(-1, 3)
        capi.normals_from_map(xyz, w, h, k)
        t0 = time.perf_counter()
        nrm, ms_dev = capi.normals_from_map(xyz, w, h, k, want_ms=True)
        dt = time.perf_counter() - t0
        W, H = w + 2 * k, h + 2 * k
        bytes_alg = w * h * 24.0 * 2 + W * H * 8.0 * 10 * 3     # map in, normals out, moment images written+read, sums written
        emit(f"N3 estimate_normals {w}x{h} k={k}", ms_total=dt * 1e3, ms_device=ms_dev, mpixel_per_s=w * h / (ms_dev * 1e3),
             device_GBps=bytes_alg / (ms_dev * 1e-3) / 1e9,
             roofline={"bound": "hbm", "kernel": "m3d::nm_box_sum_k + nm_normals_k + nm_moments_k", "achieved": bytes_alg / (ms_dev * 1e-3) / 1e9,
                       "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": bytes_alg / (ms_dev * 1e-3) / 1e9 / HBM_PEAK_GBS,
                       "note": "device time of the three kernels (HIP events); the box sums keep the reference's summation order "
                               "(a serial recurrence along every row and column), which is what holds them below the bandwidth; "
                               "the whole call is bound by the host link (map in, normals out)"},
             cpu_baseline=None if NO_CPU else n3_cpu(xyz, w, h, k))

if "N4" in which or ALL:
    # DetectBoundaryPoints on a 500 k-point planar patch (the inliers of a fit_plane), Hybrid(0.02, 30)
    rng = np.random.default_rng(3)
    nb = 500_000
    uv = rng.uniform(0, 3.0, (nb, 2))
    pp = np.c_[uv[:, 0], uv[:, 1], 0.2 * uv[:, 0] + rng.normal(0, 1e-3, nb)]
    capi.detect_boundary_points(pp[:1000], None, 2, 0.02, 30, 90.0)
    ts = []
    for _ in range(3):      # one-call entry point: median of three (the first full-size call also sizes the block free list)
        t0 = time.perf_counter()
        bidx = capi.detect_boundary_points(pp, None, 2, 0.02, 30, 90.0)
        ts.append((time.perf_counter() - t0) * 1e3)
    # per point: a hybrid search (27 cells, ~60 candidates, sorted insertion of the 30 nearest), a 3x3 eigen-problem for the
    # normal, 30 atan2 and their sort -- latency- and LDS-bound per thread; no bandwidth or issue roofline applies cleanly
    def n4_cpu():
        import oracle
        m = 40_000     # (the oracle's search is a uniform grid too, single thread)
        t0 = time.perf_counter()
        oracle.detect_boundary_points(pp[:m] * [1, 1, 1], None, 2, 0.02, 30, 90.0)
        dt_c = time.perf_counter() - t0
        return {"value": m / dt_c, "unit": "points/s", "cores": 1, "kind": "port",
                "sample": f"the first {m} points as a cloud of their own (same density along one edge: the patch is uniform), {dt_c:.1f} s; "
                          "src/boundary_detection.cpp:68-113 runs its loop under OpenMP: x cores at best", "flags": "-O3 -ffp-contract=off (no -march)"}
    # The kernel's own bound, from one counter pass (tools/pmc_boundary.sh -> profiles/r06_pmc_boundary.txt): boundary_k issues
    # N4_VALU_PER_POINT VALU + N4_LDS_PER_POINT LDS instructions per wave of 64 points (one point per LANE: the 30-neighbour insertion
    # sort and the angle sort run in LDS); the issue roofline is those instructions x 4 cycles over the launch's SIMD cycles.
    N4_VALU_PER_POINT, N4_LDS_PER_POINT = N4_COUNTS
    ms4 = sorted(ts)[1]
    n4_issue = nb / 64.0 * (N4_VALU_PER_POINT + N4_LDS_PER_POINT) * 4.0 / (1024 * 2.4e9)     # seconds if every instruction issued back to back
    emit("N4 detect_boundary_points 500k pts Hybrid(0.02, 30), normals estimated", ms=ms4, ms_first=ts[0],
         boundary_points=len(bidx), points_per_s=nb / (ms4 * 1e-3),
         roofline={"bound": "instruction issue (VALU + LDS): per point a 27-cell search with a sorted insertion of the 30 nearest, a 3x3 "
                            "eigen-problem, 30 atan2 and their sort, one point per lane -- divergent loops, nothing streams",
                   "kernel": "m3d::boundary_k", "achieved": nb / 64.0 * (N4_VALU_PER_POINT + N4_LDS_PER_POINT) / (ms4 * 1e-3) / 1e12,
                   "peak": 1024 * 2.4e9 / 4.0 / 1e12, "unit": "T wave-instructions/s (VALU + LDS issue, whole call's wall clock)",
                   "frac": n4_issue / (ms4 * 1e-3), "valu_per_point": N4_VALU_PER_POINT, "lds_per_point": N4_LDS_PER_POINT,
                   "source": "profiles/r06_pmc_boundary.txt (SQ_INSTS_VALU, SQ_INSTS_LDS of boundary_k / points)"},
         cpu_baseline=None if NO_CPU else n4_cpu())

if "C5" in which:
    n = int(os.environ.get("M3D_C5_POINTS", "10000000"))
    pts = synth.room_cloud_c5(n, 6)
    # the binding's defaults: every cluster comes back as an array of its own; the library writes the index lists into a
    # page-locked scratch the binding keeps (first call: + its allocation).  copy=False (views of a pageable array the
    # library fills through staged copies) is the slower way round: 43 against 37 ms
    t0 = time.perf_counter()
    rc, planes, clusters = capi.segment_plane_iterative(pts, 0.01, max_iteration=1000, min_ratio=0.05, seed=19)
    dt = time.perf_counter() - t0
    dts = []
    for _ in range(3):
        t0 = time.perf_counter()
        rc, planes, clusters = capi.segment_plane_iterative(pts, 0.01, max_iteration=1000, min_ratio=0.05, seed=19)
        dts.append(time.perf_counter() - t0)
    dt2 = sorted(dts)[1]
    # HBM-bound by construction (a round = a few hundred hypotheses on what is left of the cloud, then compaction + removal
    # passes over it): algorithmic bytes = per round 24 B x remaining points x 4 (RefineModel's counting and writing pass,
    # the removal's read of both copies) + 24 B x kept points x 2 (both copies written) + the 240 MB upload and transpose
    br = capi.last_segment_ms()       # the library's own clock of the last call: create / round loop / its big rounds
    rem, alg = n, 24.0 * n * 3
    alg_big = alg_tail = 0.0
    for cidx in clusters:
        b = 24.0 * rem * 4 + 24.0 * (rem - len(cidx)) * 2
        alg += b
        if rem > n / 8:
            alg_big += b
        else:
            alg_tail += b
        rem -= len(cidx)
    n_tail = max(br["n_rounds"] - br["n_big_rounds"], 1)
    t_tail = (br["rounds"] - br["big_rounds"]) * 1e-3
    emit("C5 segment_plane_iterative 10M pts (1 GPU, incl. 240 MB upload)", ms_first=dt * 1e3, ms=dt2 * 1e3, rc=rc,
         clusters=[len(c) for c in clusters][:12] + ["... %d more" % max(0, len(clusters) - 12)], planes=len(planes),
         roofline={"bound": "hbm", "kernel": "compact_count_k / compact_write_k / cull_mask_k over the remaining cloud, per round",
                   "achieved": alg / dt2 / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": alg / dt2 / 1e9 / HBM_PEAK_GBS,
                   "algorithmic_bytes": alg, "rounds": len(clusters),
                   "phases": {
                       "inside_the_library_ms": br["total"], "binding_ms": dt2 * 1e3 - br["total"],
                       "cloud_create": {"ms": br["cloud_create"], "bytes": 24.0 * n * 3,
                                        "GBps": 24.0 * n * 3 / (br["cloud_create"] * 1e-3) / 1e9,
                                        "bound": "PCIe: 240 MB from the caller's pageable array at ~52 GB/s = 4.6 ms of it"},
                       "big_rounds": {"rounds": br["n_big_rounds"], "ms": br["big_rounds"], "algorithmic_bytes": alg_big,
                                      "GBps": alg_big / (br["big_rounds"] * 1e-3) / 1e9,
                                      "frac": alg_big / (br["big_rounds"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                      "note": "rounds on more than an eighth of the cloud (the six walls, floor, ceiling)"},
                       "tail_rounds": {"rounds": n_tail, "ms": t_tail * 1e3, "us_per_round": t_tail * 1e6 / n_tail,
                                       "algorithmic_bytes": alg_tail, "GBps": alg_tail / t_tail / 1e9,
                                       "frac": alg_tail / t_tail / 1e9 / HBM_PEAK_GBS,
                                       "note": "1000 hypotheses on ~1 M clutter points each, the round's kernels back to back: ~58 us of box tests and scoring (latency-bound launches, 8 % of the (tile, hypothesis) pairs survive), ~24 us of RefineModel's compaction + the partition in creation order at 3.6 TB/s, ~8 us for the previous round's tombstone pass riding in minimal_fit_k's launch; no host wait but the records' (profiles/r03_c5_round_timeline.txt)"}},
                   "note": "whole call (PCIe upload of 240 MB and 76 MB of index lists back included)"},
         cpu_baseline=cpu("segmentation_baseline", pts, 0.01, 1000, 0.05, 19, [c for c in clusters if len(c) > n / 8], 14.0))

if "P1" in which or "P2" in which or ALL:
    # misc3d.preprocessing.farthest_point_sampling: P1 = the reference example's shape (examples/python/farthest_point_sampling.py,
    # 5 841 points x 1 000 samples), P2 = 1 M synthetic points x 10 000 samples
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from fps_ref_util import build_ref

    def fps_cpu(pts, S, steps):
        """the serial restatement of the reference's loop (tests/cpp/fps_ref.c, gcc -O2 -ffp-contract=off), timed on a bounded
        number of steps and scaled linearly to S (every step is one full pass over the N points: constant cost)"""
        if NO_CPU:
            return None
        ref = build_ref(tempfile.mkdtemp())
        ref(pts, 2)
        t0 = time.perf_counter()
        ref(pts, steps)
        dt = time.perf_counter() - t0
        return {"value": dt / steps * S * 1e3, "unit": "ms (scaled)", "cores": 1, "kind": "port",
                "sample": f"{steps} of {S} steps timed ({dt * 1e3:.1f} ms), scaled linearly: the reference's loop is serial, "
                          "with no OpenMP (src/filter.cpp:13-52)", "ns_per_point_update": dt / (steps * len(pts)) * 1e9,
                "flags": "-O2 -ffp-contract=off"}

    for tag, n, S, paths in (("P1", 5841, 1000, (1, 2, 3)), ("P2", 1_000_000, 10_000, (2, 3))):
        if not (tag in which or ALL):
            continue
        pts = np.random.default_rng(17).uniform(-1, 1, (n, 3))
        rows = {}
        for path in paths:
            capi.fps_force_path(path)
            try:
                capi.farthest_point_sampling(pts, S)   # (sizes the lane's block free list)
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    idx, st = capi.farthest_point_sampling(pts, S, stats=True)
                    ts.append(((time.perf_counter() - t0) * 1e3, st))
            finally:
                capi.fps_force_path(0)
            ms, st = sorted(ts, key=lambda r: r[0])[1]
            rows[{1: "single", 2: "pruned", 3: "dense"}[path]] = {
                "ms": ms, "ms_device": st["ms_device"], "ms_in_library": st["ms_total"], "pruned_fraction": st["pruned_fraction"],
                "tiles_updated": st["tiles_updated"], "tile_steps": st["tile_steps"]}
        default = capi.farthest_point_sampling(pts, S, stats=True)[1]
        path_name = {1: "single", 2: "pruned", 3: "dense"}[default["path"]]
        best = rows[path_name]
        if tag == "P1":
            roofline = {"bound": "latency: one workgroup, one step = update + wave argmax + one barrier",
                        "kernel": "m3d::fps_single_k<8>", "achieved": best["ms_device"] * 1e3 / (S - 1), "unit": "us per step",
                        "note": "a step's serial chain (8 point updates, 6 shuffle levels, LDS, __syncthreads, 16-way reduce) "
                                "bounds it, not bandwidth: the cloud sits in registers"}
        else:
            dense_bytes = 32.0 * n * (S - 1)
            d = rows["dense"]
            roofline = {"bound": "pruned: one kernel boundary per sample (~1.5 us, MI355X_MICROARCH.md row boundary); "
                                 "dense: HBM, 32 B per point per step",
                        "kernel": "m3d::fps_step_k", "launches": S - 1,
                        "pruned_us_per_step": rows["pruned"]["ms_device"] * 1e3 / (S - 1),
                        "launch_floor_ms": 1.5e-3 * (S - 1),
                        "frac_pruned_vs_launch_floor": 1.5e-3 * (S - 1) / rows["pruned"]["ms_device"],
                        "dense_achieved_GBps": dense_bytes / (d["ms_device"] * 1e-3) / 1e9, "peak": HBM_PEAK_GBS,
                        "dense_frac": dense_bytes / (d["ms_device"] * 1e-3) / 1e9 / HBM_PEAK_GBS, "unit": "GB/s (dense)"}
        emit(f"{tag} farthest_point_sampling {n} pts x {S} samples", ms=best["ms"], ms_device=best["ms_device"], path=path_name,
             pruned_fraction=best["pruned_fraction"], paths=rows, roofline=roofline,
             cpu_baseline=fps_cpu(pts, S, 200 if n < 100_000 else 20))

if any(t in which for t in ("S1", "S2", "S3", "S4")) or ALL:
    # misc3d.segmentation.ProximityExtractor: S1 = the reference example (examples/python/segmentation.py: the golden cloud
    # voxel-averaged at 0.01, PCA normals, DistanceNormals(0.02, 30), radius 0.02, min 100), S2 = the raw 40 458-point PLY with
    # Distance(0.01) at r = 0.01, S3 = 1 M uniform points, S4 = 10 M points on the walls of boxes in a 40 m room (the grid's
    # 2^27-cell cap coarsens its cells)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from proximity_ref_util import golden_ply, pca_normals, voxel_average

    def prox_cpu(xyz, radius, kind, dist, ang, nrm, scale=1.0):
        """scipy cKDTree pairs + the evaluator in numpy + csgraph.connected_components (the pair search is single-threaded)"""
        if NO_CPU:
            return None
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        from scipy.spatial import cKDTree
        t0 = time.perf_counter()
        p = cKDTree(xyz).query_pairs(radius, output_type="ndarray")
        a, b = p[:, 0], p[:, 1]
        keep = np.ones(len(a), bool)
        if kind != "normals":
            d = xyz[a] - xyz[b]
            keep &= np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < dist
        if kind != "distance":
            dot = (nrm[a, 0] * nrm[b, 0] + nrm[a, 1] * nrm[b, 1]) + nrm[a, 2] * nrm[b, 2]
            keep &= np.arccos(np.clip(dot, -1, 1)) <= np.radians(ang)
        g = coo_matrix((np.ones(keep.sum(), np.int8), (a[keep], b[keep])), shape=(len(xyz), len(xyz)))
        connected_components(g, directed=False)
        dt = time.perf_counter() - t0
        return {"value": dt * 1e3 * scale, "unit": "ms" if scale == 1.0 else "ms (scaled)", "cores": 1,
                "kind": "scipy cKDTree.query_pairs + csgraph.connected_components",
                "pairs": int(len(a)), **({"sample": f"1/{scale:g} of the points timed, scaled linearly"} if scale != 1.0 else {})}

    def room(n, seed=5):
        rng = np.random.default_rng(seed)
        lo = rng.uniform(0, 38, (400, 3)) * [1, 1, 0.1]
        hi = lo + rng.uniform(0.3, 2.0, (400, 3))
        box = rng.integers(0, 400, n)
        face = rng.integers(0, 6, n)
        u = rng.uniform(0, 1, (n, 3))
        pts = lo[box] + u * (hi[box] - lo[box])
        ax = face % 3
        pts[np.arange(n), ax] = np.where(face < 3, lo[box, ax], hi[box, ax])
        return pts

    cases = []
    if "S1" in which or ALL:
        d = voxel_average(golden_ply(), 0.01)
        cases.append(("S1 proximity reference example", d, 0.02, "distance_normals", 0.02, 30.0, pca_normals(d, 0.02), 100, 1.0))
    if "S2" in which or ALL:
        cases.append(("S2 proximity golden PLY r=0.01", golden_ply(), 0.01, "distance", 0.01, 0.0, None, 1, 1.0))
    if "S3" in which or ALL:
        cases.append(("S3 proximity 1M uniform", np.random.default_rng(3).uniform(0, 1, (1_000_000, 3)), 0.008, "distance",
                      0.008, 0.0, None, 1, 1.0))
    if "S4" in which or ALL:
        cases.append(("S4 proximity 10M room", room(10_000_000), 0.02, "distance", 0.02, 0.0, None, 100, 10.0))
    for name, xyz, r, kind, dist, ang, nrm, mn, scale in cases:
        capi.proximity_segment(xyz, r, kind, dist, ang, nrm, mn)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            off, idx, lab, st = capi.proximity_segment(xyz, r, kind, dist, ang, nrm, mn, stats=True)
            ts.append(((time.perf_counter() - t0) * 1e3, st))
        ms, st = sorted(ts, key=lambda t: t[0])[1]
        sub = xyz[: len(xyz) // int(scale)] if scale != 1.0 else xyz
        emit(name, n=len(xyz), radius=r, evaluator=kind, clusters=len(off) - 1, ms=ms, ms_in_library=st["ms_total"],
             ms_device=st["ms_device"], ms_host_order=st["ms_order"], components=st["components"], cell_edge=st["cell_edge"],
             cell_coarsened=st["cell_edge"] / (1.001 * r),
             cpu_baseline=prox_cpu(sub, r, kind, dist, ang, None if nrm is None else nrm[: len(sub)], scale))

if any(t in which for t in ("K1", "K2", "K3", "K4")) or ALL:
    # misc3d.common.KNearestSearch: K1 = every src descriptor's 10 nearest dst descriptors (synth.registration_pair_c4),
    # K2 = 1 000 single-query search_knn(q, 10) calls on that index, K3 = every point's 30 nearest among 1 M (grid path)
    # with a tile-path A/B on a 100 k subset, K4 = 1 000 queries x k = 1 000 on 50 000 x 33 (select path)
    import misc3d_amd as m3d

    def knn_cpu(data, q, k, sample):
        """scipy cKDTree.query(k, workers=16) on `sample` of the queries, scaled linearly (build included once)"""
        if NO_CPU:
            return None
        from scipy.spatial import cKDTree
        t0 = time.perf_counter()
        tree = cKDTree(data)
        t1 = time.perf_counter()
        tree.query(q[:sample], k, workers=16)
        t2 = time.perf_counter()
        scale = len(q) / min(sample, len(q))
        return {"value": ((t1 - t0) + (t2 - t1) * scale) * 1e3, "unit": "ms" if scale == 1.0 else "ms (scaled)", "cores": 16,
                "kind": "scipy cKDTree(data).query(q, k, workers=16)", "build_ms": (t1 - t0) * 1e3,
                **({"sample": f"{min(sample, len(q))} of {len(q)} queries timed, scaled linearly"} if scale != 1.0 else {})}

    def knn_roofline(st, dim):
        """tile / select paths: fp64 VALU issue, 3 lane-ops (sub, mul, add) per pair-dim at the 39.3 T lane-op/s peak"""
        ops = 3.0 * st["pair_dims"]
        return {"bound": "fp64 valu-issue", "kernel": "m3d::knn_tile_k + knn_merge_k", "lane_ops": ops,
                "floor_ms": ops / (FP64_VALU_PEAK_TOPS * 1e12) * 1e3, "ms_device": st["ms_device"],
                "achieved": ops / (st["ms_device"] * 1e-3) / 1e12, "peak": FP64_VALU_PEAK_TOPS,
                "unit": "T lane-ops/s", "frac": ops / (st["ms_device"] * 1e-3) / (FP64_VALU_PEAK_TOPS * 1e12)}

    def knn_timed(ix, q, k, reps=3, path=0):
        capi.knn_force_path(path)
        try:
            ix.search(q[: min(len(q), 64)], k)
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                out = ix.search(q, k, want_d2=False, stats=True)
                ts.append(((time.perf_counter() - t0) * 1e3, out))
        finally:
            capi.knn_force_path(0)
        ms, out = sorted(ts, key=lambda t: t[0])[len(ts) // 2]
        return ms, out[0], out[-1]

    c4 = None
    if "K1" in which or "K2" in which or ALL:
        c4 = synth.registration_pair_c4(200_000, seed=5)
        fs, fd = np.ascontiguousarray(c4["feat_src"]), np.ascontiguousarray(c4["feat_dst"])
    if "K1" in which or ALL:
        ix = capi.KnnIndex(fd)
        ms, idx, st = knn_timed(ix, fs, 10)
        emit("K1 knn 200k x 200k x 33 k=10 batched", n=len(fd), m=len(fs), dim=33, k=10, ms=ms, ms_in_library=st["ms_total"],
             ms_device=st["ms_device"], path=st["path"], pair_dims=st["pair_dims"], roofline=knn_roofline(st, 33),
             cpu_baseline=knn_cpu(fd, fs, 10, 2000))
        ix.close()
    if "K2" in which or ALL:
        s = m3d.common.KNearestSearch(fd.T)
        qs = fs[:1000]
        s.search_knn(qs[0], 10)
        t0 = time.perf_counter()
        for q in qs:
            s.search_knn(q, 10)
        per = (time.perf_counter() - t0) * 1e3 / len(qs)
        ix = capi.KnnIndex(fd)
        _, _, st = knn_timed(ix, qs[:1], 10, reps=5)
        ix.close()
        cpu_b = None
        if not NO_CPU:
            from scipy.spatial import cKDTree
            tree = cKDTree(fd)
            t0 = time.perf_counter()
            for q in qs[:50]:
                tree.query(q, 10)
            cpu_b = {"value": (time.perf_counter() - t0) * 1e3 / 50, "unit": "ms per call", "cores": 1,
                     "kind": "scipy cKDTree.query(q, 10), one query per call (tree built beforehand), 50 calls timed"}
        emit("K2 knn 1000 single-query search_knn(q, 10) on 200k x 33", n=len(fd), dim=33, k=10, calls=len(qs),
             ms_per_call=per, ms_device_one_query=st["ms_device"], roofline=knn_roofline(st, 33), cpu_baseline=cpu_b)
    if "K3" in which or ALL:
        pts = np.random.default_rng(3).uniform(0, 1, (1_000_000, 3))
        ix = capi.KnnIndex(pts)
        ms, idx, st = knn_timed(ix, pts, 30)
        sub = np.ascontiguousarray(pts[:100_000])
        ixs = capi.KnnIndex(sub)
        rows = {}
        for name, path in (("grid", capi.KNN_PATH_GRID), ("tile", capi.KNN_PATH_TILE)):
            pms, pidx, pst = knn_timed(ixs, sub, 30, path=path)
            rows[name] = {"ms": pms, "ms_device": pst["ms_device"], "pair_dims": pst["pair_dims"], "path": pst["path"]}
            rows[name]["idx"] = pidx
        same = bool(np.array_equal(rows["grid"].pop("idx"), rows["tile"].pop("idx")))
        emit("K3 knn 1M x 3 every point's 30 nearest (grid)", n=len(pts), m=len(pts), dim=3, k=30, ms=ms,
             ms_in_library=st["ms_total"], ms_device=st["ms_device"], path=st["path"], pair_dims=st["pair_dims"],
             pairs_per_query=st["pair_dims"] / 3 / len(pts), ab_100k=rows, ab_equal=same,
             roofline={"bound": "none modelled (grid path: LDS list updates and cell walks)", "tile_path_100k": knn_roofline(
                 {"pair_dims": rows["tile"]["pair_dims"], "ms_device": rows["tile"]["ms_device"]}, 3)},
             cpu_baseline=knn_cpu(pts, pts, 30, 100_000))
        ix.close()
        ixs.close()
    if "K4" in which or ALL:
        rng = np.random.default_rng(4)
        data = rng.random((50_000, 33))
        q = rng.random((1000, 33))
        ix = capi.KnnIndex(data)
        ms, idx, st = knn_timed(ix, q, 1000)
        emit("K4 knn 50k x 33, 1000 queries, k=1000 (select)", n=len(data), m=len(q), dim=33, k=1000, ms=ms,
             ms_in_library=st["ms_total"], ms_device=st["ms_device"], path=st["path"], pair_dims=st["pair_dims"],
             pages=st["launches"] // 2, roofline=knn_roofline(st, 33), cpu_baseline=knn_cpu(data, q, 1000, 1000))
        ix.close()

if "F1" in which or ALL:
    # fragment preprocessing (PreProcessFragments): normals Hybrid(2 voxel, 30) + FPFH Hybrid(5 voxel, 100) on the three-surface
    # cloud of the FPFH tests; cpu_baseline = the plain-C brute-force restatement (tests/cpp/fpfh_ref.c) under OpenMP on 16
    # threads -- NOT Open3D's KD-tree implementation, which is not in the image
    import tempfile
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import fpfh_ref_util as fpfh_util
    for n, voxel in ((50_000, 0.02), (200_000, 0.01)):
        pts, _ = fpfh_util.three_surface_cloud(n, seed=1)
        for _ in range(2):
            capi.preprocess_fragment(pts, voxel)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            st = capi.preprocess_fragment(pts, voxel, stats=True)[2]
            ts.append(((time.perf_counter() - t0) * 1e3, st))
        ms, st = sorted(ts, key=lambda t: t[0])[1]
        cpu = None
        if not NO_CPU:
            os.environ.setdefault("OMP_NUM_THREADS", "16")
            ref = fpfh_util.build_ref(tempfile.mkdtemp())
            t0 = time.perf_counter()
            ref.preprocess(pts, voxel)
            cpu = {"ms": (time.perf_counter() - t0) * 1e3, "what": "tests/cpp/fpfh_ref.c: brute-force restatement, OpenMP, 16 threads"}
        emit(f"F1 preprocess_fragment {n} points, voxel {voxel}", n=n, voxel=voxel, ms=ms, ms_in_library=st["ms_total"],
             ms_device=st["ms_device"], ms_upload=st["ms_upload"], ms_search=st["ms_search"], ms_normals=st["ms_normals"],
             ms_spfh=st["ms_spfh"], ms_fpfh=st["ms_fpfh"], pairs=st["pairs"], pairs_seen=st["pairs_seen"],
             launches=st["launches"], cpu_baseline=cpu)

if any(t in which for t in ("V1", "V2", "V3")) or ALL:
    # misc3d.preprocessing.voxel_down_sample from host arrays: the 1 M-point scene bench.py fits (synth.plane_cloud_c2) at voxel
    # sizes 0.005 (V1) and 0.02 (V2) of the scene's largest extent, and the three-level call {v, v/2, v/4} from v = 0.02 (V3).
    # Median of 25 calls after 5 warm-up calls; the split upload / device / download is m3d_voxel_stats' (HIP events on the
    # lane's stream); spread = (min, max) of the wall clock.
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from voxel_ref_util import build_ref as voxel_build_ref

    pts = np.ascontiguousarray(synth.plane_cloud_c2(1_000_000, seed=2))
    scale = float((pts.max(axis=0) - pts.min(axis=0)).max())
    HOST_LINK_GBS = 64.0   # PCIe 5 x16, one direction, nominal

    def voxel_cpu(sizes):
        """tests/cpp/voxel_ref.c (gcc -O2 -ffp-contract=off): the reference's algorithm, one thread and a hash map -- x1 core, as
        the reference runs it; the whole call, the fastest of 3"""
        if NO_CPU:
            return None
        ref = voxel_build_ref(tempfile.mkdtemp())
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            for s in sizes:
                ref(pts, s)
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"value": min(ts), "unit": "ms", "cores": 1, "kind": "port", "flags": "-O2 -ffp-contract=off",
                "note": "x1 core, as the reference runs it (one serial pass over a hash map per level)"}

    for tag, sizes in (("V1", [0.005 * scale]), ("V2", [0.02 * scale]), ("V3", [0.02 * scale, 0.01 * scale, 0.005 * scale])):
        if not (tag in which or ALL):
            continue
        call = (lambda: capi.voxel_down_sample_multi(pts, sizes, stats=True)) if len(sizes) > 1 else \
               (lambda: capi.voxel_down_sample(pts, sizes[0], stats=True))
        for _ in range(5):
            call()
        runs = []
        for _ in range(25):
            t0 = time.perf_counter()
            _, st = call()
            runs.append(((time.perf_counter() - t0) * 1e3, st))
        runs.sort(key=lambda r: r[0])
        ms, st = runs[len(runs) // 2]
        med = lambda k: float(np.median([r[1][k] for r in runs]))   # noqa: E731
        up_bytes, down_bytes = 24.0 * len(pts), 24.0 * st["n_voxels"]
        emit(f"{tag} voxel_down_sample 1M points, voxel {' / '.join(f'{s / scale:g}' for s in sizes)} of the scene",
             n=len(pts), voxel_sizes=sizes, voxels=st["n_voxels"], ms=ms, ms_spread=[runs[0][0], runs[-1][0]], runs=len(runs),
             warmup=5, ms_in_library=med("ms_total"), ms_upload=med("ms_upload"), ms_device=med("ms_device"),
             ms_download=med("ms_download"), sort_passes=st["sort_passes"], path=st["path"],
             roofline={"bound": "host link: every byte moves once (24 B per point up, 24 B per voxel down)",
                       "bytes_up": up_bytes, "bytes_down": down_bytes,
                       "link_floor_ms": (up_bytes + down_bytes) / (HOST_LINK_GBS * 1e9) * 1e3, "link_peak_GBps": HOST_LINK_GBS,
                       "achieved_GBps_call": (up_bytes + down_bytes) / (ms * 1e-3) / 1e9,
                       "hbm_floor_ms": (up_bytes + down_bytes) / (HBM_PEAK_GBS * 1e9) * 1e3,
                       "device_ms_over_hbm_floor": med("ms_device") / ((up_bytes + down_bytes) / (HBM_PEAK_GBS * 1e9) * 1e3),
                       "note": "the device part is many small launches over 4-byte arrays (hash insert, scan, 8-bit sort passes, "
                               "one wave per voxel for the ordered sums) and two round trips (bounds, voxel count), not a "
                               "streaming kernel: it is not expected near the HBM floor"},
             cpu_baseline=voxel_cpu(sizes))

if "I1" in which or "I2" in which or ALL:
    # point-to-plane ICP and the multi-scale driver ("Multi-scale ICP").  The pair is the C4 shape -- the six
    # patches of synth.registration_pair_c4 -- with analytic normals (tests/icp_ref_util.icp_pair: synth has none).
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import icp_ref_util as icp_util
    import misc3d_amd as m3d

    if "I1" in which or ALL:
        # I1: both estimators from the same process, alternating.  A whole call (30 iterations allowed, the default criteria), and
        # the time of ONE iteration = (call with 40 iterations - call with 10) / 30 with both relative criteria at 0 so that
        # every iteration runs: set-up (two uploads, the target grid and its neighbour lists) cancels.
        n = 200_000
        p = icp_util.icp_pair(n, seed=5, sigma=0.002)
        init = icp_util.offset_pose(p["T"], 0.3, (0.003, -0.002, 0.002))

        def plane(it, rel):
            return capi.registration_icp_plane(p["src"], p["dst"], p["dst_normals"], 0.02, init, it, rel, rel)

        def plane_l1(it, rel):
            return capi.registration_icp_plane(p["src"], p["dst"], p["dst_normals"], 0.02, init, it, rel, rel, l1=True)

        def point(it, rel):
            return capi.registration_icp(p["src"], p["dst"], 0.02, init, it, rel, rel)
        for fn in (plane, plane_l1, point):
            fn(30, 1e-6)
        rows = {"plane": {}, "plane_l1": {}, "point": {}}
        for rep in range(7):
            for name, fn in (("plane", plane), ("plane_l1", plane_l1), ("point", point)):
                for key, it, rel in (("call", 30, 1e-6), ("it10", 10, 0.0), ("it40", 40, 0.0)):
                    t0 = time.perf_counter()
                    T, st = fn(it, rel)
                    rows[name].setdefault(key, []).append(((time.perf_counter() - t0) * 1e3, st, T))
        out = {}
        for name in rows:
            med = {k: sorted(v, key=lambda r: r[0])[len(v) // 2] for k, v in rows[name].items()}
            assert med["it10"][1]["iterations"] == 10 and med["it40"][1]["iterations"] == 40
            out[name] = {"ms_call": med["call"][0], "ms_call_spread": [min(r[0] for r in rows[name]["call"]), max(r[0] for r in rows[name]["call"])],
                         "iterations": med["call"][1]["iterations"], "fitness": med["call"][1]["fitness"],
                         "rmse": med["call"][1]["inlier_rmse"], "pose_err": float(np.abs(med["call"][2] - p["T"]).max()),
                         "ms_10_iterations": med["it10"][0], "ms_40_iterations": med["it40"][0],
                         "us_per_iteration": (med["it40"][0] - med["it10"][0]) / 30.0 * 1e3}
        emit("I1 registration_icp_plane vs registration_icp, 200k x 200k, 0.02 (alternating, medians of 7)", n=n,
             point_to_plane=out["plane"], point_to_plane_l1=out["plane_l1"], point_to_point=out["point"],
             launches_per_iteration={"point_to_plane": "2 (+ the completion word's)", "point_to_point": "5 + 3 final reductions (+ the completion word's)"},
             roofline={"bound": "latency: an iteration is a dependent chain of short launches, one 240-byte copy and one host wait",
                       "us_per_iteration_plane": out["plane"]["us_per_iteration"],
                       "us_per_iteration_plane_l1": out["plane_l1"]["us_per_iteration"], "us_per_iteration_point": out["point"]["us_per_iteration"]},
             cpu_baseline=None)

    if "I2" in which or ALL:
        n = 50_000
        p = icp_util.icp_pair(n, seed=6, sigma=0.001)
        v = 0.02
        init = icp_util.offset_pose(p["T"], 1.0, (0.008, -0.005, 0.006))
        tgt = (p["dst"], p["dst_normals"])
        # the coloured line: the same pair with the smooth colour field of the coloured-ICP tests on both clouds
        import colored_icp_ref_util as colored_util
        sc, dc = colored_util.colors_of(p)
        for method in ("point_to_plane", "point_to_point", "colored"):
            src_m, tgt_m = ((p["src"], None, sc), (p["dst"], p["dst_normals"], dc)) if method == "colored" else (p["src"], tgt)
            for _ in range(3):
                m3d.reconstruction.refine_fragment_pair(src_m, tgt_m, v, init, method)
            runs = []
            for _ in range(15):
                t0 = time.perf_counter()
                T, info, lv = m3d.reconstruction.refine_fragment_pair(src_m, tgt_m, v, init, method, stats=True)
                runs.append(((time.perf_counter() - t0) * 1e3, lv, T, info))
            runs.sort(key=lambda r: r[0])
            ms, lv, T, info = runs[len(runs) // 2]
            med = lambda l, k: float(np.median([r[1][l][k] for r in runs]))   # noqa: E731
            emit(f"I2 refine_fragment_pair 50k-point fragments, voxel {v}, {method} (median of 15)", n=n, voxel=v, ms=ms,
                 ms_spread=[runs[0][0], runs[-1][0]], pose_err=float(np.abs(T - p["T"]).max()), info_55=float(info[5, 5]),
                 levels=[{"n_src": l["n_src"], "n_dst": l["n_dst"], "iterations": l["icp"]["iterations"],
                          "fitness": l["icp"]["fitness"], "ms_down_sample": med(i, "ms_down_sample"), "ms_icp": med(i, "ms_icp"),
                          "ms_information": med(i, "ms_information")} for i, l in enumerate(lv)],
                 roofline={"bound": "latency + host link: three levels through host arrays (download of every level, upload into the "
                                    "ICP call), a grid per level, then one pass over the original clouds"},
                 cpu_baseline=None)

if any(t in which for t in ("R1", "R2", "R3")) or ALL:
    # pose_estimation.RayCastRenderer ("Ray casting") through the C ABI, host arrays in and out.  The mesh is
    # the reference example's obj.ply (tests/golden/raycast_obj.npz, 11 678 triangles) scaled by 0.001.  Median of 15 calls after
    # 3 warm-up calls; the split is m3d_raycast_stats' (HIP events on the lane's stream); pruning = rule-3 pair tests run over
    # rays x triangles.  cpu_baseline = the plain-C BRUTE FORCE over every pair (tests/cpp/raycast_ref.c) under OpenMP on 16
    # threads -- NOT Embree, which the reference uses and which is not in the image.
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import raycast_ref_util as ray_util

    mesh, ex_poses, ex_cam = ray_util.golden_obj(1)

    def ray_line(tag, name, meshes, frames, cam, reps=15, baseline=False):
        for _ in range(3):
            capi.raycast_pinhole(meshes, frames, cam)
        runs = []
        for _ in range(reps):
            t0 = time.perf_counter()
            res, st = capi.raycast_pinhole(meshes, frames, cam, stats=True)
            runs.append(((time.perf_counter() - t0) * 1e3, st))
        runs.sort(key=lambda r: r[0])
        ms, st = runs[len(runs) // 2]
        med = lambda k: float(np.median([r[1][k] for r in runs]))   # noqa: E731
        cpu, extra = None, {}
        if baseline and not NO_CPU:
            os.environ.setdefault("OMP_NUM_THREADS", "16")
            ref = ray_util.build_ref(tempfile.mkdtemp(), openmp=True)
            t0 = time.perf_counter()
            exp = ref(meshes, frames[0], cam)
            cpu = {"value": (time.perf_counter() - t0) * 1e3, "unit": "ms", "kind": "brute force, not Embree",
                   "what": "tests/cpp/raycast_ref.c: every (ray, triangle) pair, gcc -O2 -ffp-contract=off -fopenmp, 16 threads"}
            extra = {"equal_to_brute_force_bit_for_bit": bool(ray_util.same({k: v[0] for k, v in res.items()}, exp)),
                     "clause": exp["counts"]}
        emit(f"{tag} {name}", width=cam[0], height=cam[1], meshes=len(meshes), frames=len(frames), triangles=st["n_triangles"],
             nodes=st["n_nodes"], rays=st["n_rays"], ms=ms, ms_spread=[runs[0][0], runs[-1][0]], runs=reps, warmup=3,
             ms_per_frame=ms / len(frames), ms_in_library=med("ms_total"), ms_upload=med("ms_upload"), ms_build=med("ms_build"),
             ms_traverse=med("ms_traverse"), ms_download=med("ms_download"), pair_tests=st["pair_tests"],
             nodes_visited=st["nodes_visited"], pair_tests_per_ray=st["pair_tests"] / st["n_rays"],
             nodes_visited_per_ray=st["nodes_visited"] / st["n_rays"],
             pruning=st["pair_tests"] / (float(st["n_rays"]) * max(st["n_triangles"], 1)),
             rays_per_second_traversal=st["n_rays"] / (med("ms_traverse") * 1e-3),
             roofline={"bound": "latency and divergence: a ray walks ~tens of dependent 64-byte node reads, the lanes of a wave "
                                "diverge below the first levels; neither the HBM nor the VALU peak is a meaningful ceiling here",
                       "share_of_peak": "not measured"},
             cpu_baseline=cpu, **extra)

    if "R1" in which or ALL:
        ray_line("R1", "ray cast, the reference example: 640 x 480, obj.ply at its two poses", [mesh, mesh], [list(ex_poses)], ex_cam,
                 baseline=True)
    if "R2" in which or ALL:
        # 64 instances on an 8 x 8 lattice that fills a 1920 x 1080 view of the example's focal length x 3
        cam = (1920, 1080, ex_cam[2] * 3, ex_cam[3] * 3, 959.5, 539.5)
        poses = []
        for k in range(64):
            T = ex_poses[k % 2].copy()
            T[:3, 3] = ((k % 8 - 3.5) * 0.085, (k // 8 - 3.5) * 0.047, 1.0 + 0.01 * (k % 5))
            poses.append(T)
        ray_line("R2", "ray cast, 1920 x 1080, 64 instances of obj.ply", [mesh] * 64, [poses], cam)
    if "R3" in which or ALL:
        frames = []
        for f in range(100):
            a, b = ex_poses[0].copy(), ex_poses[1].copy()
            a[0, 3] += 0.001 * f
            b[1, 3] -= 0.001 * f
            frames.append([a, b])
        ray_line("R3", "ray cast, a 100-frame batch of the reference example (one call)", [mesh, mesh], frames, ex_cam, reps=7)

def ppf_median(fn, reps=5):
    """PV1, PC1, PV2: one warm-up call, then the median of `reps` timed ones -> (ms, that call's result)"""
    fn()
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        runs.append(((time.perf_counter() - t0) * 1e3, r))
    runs.sort(key=lambda t: t[0])
    return runs[len(runs) // 2]


if "PV1" in which or ALL:
    # pose_estimation.PPFVoting ("PPF voting") through the C ABI: the table of a 2 000-point model (box
    # family of the PPF tests) and the vote of a 20 000-point scene -- the posed model in 18 000 points of clutter -- at ratio 0.6:
    # 12 000 reference points.  Median of 5 calls after 1 warm-up; the vote once more with its accumulators forced into device
    # memory (the A/B of the LDS path).  cpu_baseline = the contract's C restatement (tests/cpp/ppf_ref.c) under OpenMP on 16
    # threads: the table whole, the vote on every tenth reference point, scaled.
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ppf_ref_util as ppf_util

    pts, nrm, diameter, r_min = ppf_util.model_case("box", 2000)
    sp, sn, _ = ppf_util.scene_of(pts, nrm, ppf_util.pose(1), 18_000, 1)
    refs = np.sort(np.random.default_rng(1).permutation(len(sp))[: int(0.6 * len(sp))])

    ms_table, model = ppf_median(lambda: capi.PpfModel(pts, nrm, diameter, r_min))
    ms_vote, (res, st) = ppf_median(lambda: model.vote(sp, sn, refs, stats=True))
    capi.ppf_force(True, 0)
    try:
        ms_vote_dev, (res_dev, st_dev) = ppf_median(lambda: model.vote(sp, sn, refs, stats=True))
    finally:
        capi.ppf_force(False, 0)
    cpu_b = None
    if not NO_CPU:
        os.environ.setdefault("OMP_NUM_THREADS", "16")
        ref = ppf_util.PpfRef(tempfile.mkdtemp(), openmp=True)
        t0 = time.perf_counter()
        rm = ref.model(pts, nrm, diameter, r_min)
        t1 = time.perf_counter()
        rv = rm.vote(sp, sn, refs[::10])
        t2 = time.perf_counter()
        cpu_b = {"ms_table": (t1 - t0) * 1e3, "ms_vote": (t2 - t1) * 1e3 * len(refs) / len(refs[::10]), "unit": "ms",
                 "vote_sampled": "every 10th reference point, scaled by the count", "increments_sampled": rv["increments"],
                 "what": "tests/cpp/ppf_ref.c: the contract's restatement, gcc -O2 -ffp-contract=off -fopenmp, 16 threads"}
    emit("PV1 ppf table 2 000 points + vote 20 000-point scene, 12 000 reference points", n=len(pts), m=len(sp), n_ref=len(refs),
         ms_table=ms_table, ms_vote=ms_vote, ms_vote_device=st["ms_device"], path=st["path"], groups=st["groups"],
         launches=st["launches"], neighbours_visited=st["neighbours_visited"], increments=st["increments"], maxima=len(res["votes"]),
         increments_per_second=st["increments"] / (st["ms_device"] * 1e-3),
         device_memory_path={"ms_vote": ms_vote_dev, "ms_vote_device": st_dev["ms_device"], "path": st_dev["path"],
                             "same_result": bool(all(np.array_equal(res[k], res_dev[k]) for k in res))},
         roofline={"bound": "atomic increments (LDS or L2) and the divergent walk over table cells; no HBM or VALU ceiling is meaningful",
                   "share_of_peak": "not measured"},
         cpu_baseline=cpu_b)

if "PC1" in which or ALL:
    # PPF pose clustering ("PPF pose clustering") on PV1's model and scene: the vote's raw poses through
    # m3d_ppf_cluster_poses (median of 5 calls after 1 warm-up), then the whole m3d_ppf_estimate with its own split into vote,
    # cluster, refine and host (median of 3 by total; score_thresh 0 so that the list is not empty: the reference's expected
    # votes assume its own sampling).  cpu_baseline = the contract's C restatement of K1 - K6 (tests/cpp/ppf_cluster_ref.c)
    # under OpenMP on 16 threads, on the same raw poses.
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ppf_cluster_ref_util as pc_util
    import ppf_ref_util as ppf_util

    pts, nrm, diameter, r_min = ppf_util.model_case("box", 2000)
    sp, sn, _ = ppf_util.scene_of(pts, nrm, ppf_util.pose(1), 18_000, 1)
    refs = np.sort(np.random.default_rng(1).permutation(len(sp))[: int(0.6 * len(sp))])

    model = capi.PpfModel(pts, nrm, diameter, r_min)
    raw = model.vote(sp, sn, refs)
    ms_cluster, cl = ppf_median(lambda: capi.ppf_cluster_poses(raw["poses"], raw["votes"], model=model), 5)
    ms_estimate, est = ppf_median(lambda: capi.ppf_estimate(model, sp, sn, refs, score_thresh=0.0), 3)
    ms_norefine, est0 = ppf_median(lambda: capi.ppf_estimate(model, sp, sn, refs, score_thresh=0.0, refine_method="NoRefine"), 3)
    es = est["stats"]
    cpu_b = None
    if not NO_CPU:
        os.environ.setdefault("OMP_NUM_THREADS", "16")
        ref = pc_util.PcRef(tempfile.mkdtemp(), openmp=True)
        t0 = time.perf_counter()
        rc = ref.cluster(raw["poses"], raw["votes"], 0.05 * diameter, 12.0 / 180.0 * np.pi)
        cpu_b = {"ms_cluster": (time.perf_counter() - t0) * 1e3, "unit": "ms",
                 "same_integers": bool(all(np.array_equal(np.asarray(rc[k]).astype(np.int64), np.asarray(cl[k]).astype(np.int64)) for k in pc_util.INT_KEYS)),
                 "what": "tests/cpp/ppf_cluster_ref.c: the contract's restatement of K1 - K6, gcc -O2 -ffp-contract=off -fopenmp, 16 threads"}
    st = cl["stats"]
    emit("PC1 ppf pose clustering of PV1's raw poses + the whole m3d_ppf_estimate", n=len(pts), m=len(sp), n_ref=len(refs),
         raw_poses=len(raw["votes"]), n_valid=st["n_valid"], clusters_t=st["clusters_t"], clusters_r=st["clusters_r"],
         min_num_pt_t=cl["min_num_pt_t"], pair_tests=st["pair_tests"], launches=st["launches"], splits=st["splits"],
         ms_cluster=ms_cluster, ms_cluster_device=st["ms_device"], pair_tests_per_second=st["pair_tests"] / (st["ms_device"] * 1e-3),
         estimate={"ms_total": ms_estimate, "ms_vote": es["ms_vote"], "ms_cluster": es["ms_cluster"], "ms_refine": es["ms_refine"],
                   "ms_host": es["ms_host"], "icp_calls": es["icp_calls"], "icp_iterations": es["icp_iterations"],
                   "results": len(est["votes"]), "top_votes": int(est["votes"][0]) if len(est["votes"]) else 0,
                   "top_score": float(est["scores"][0]) if len(est["votes"]) else 0.0,
                   "top_pose_error": float(np.abs(est["poses"][0] - ppf_util.pose(1)).max()) if len(est["votes"]) else None,
                   "ms_total_no_refine": ms_norefine},
         roofline={"bound": "fp64 VALU of the all-pairs loops (three launches a level) and the LDS broadcast feeding them",
                   "share_of_peak": "not measured"},
         cpu_baseline=cpu_b)

if "PV2" in which or ALL:
    # pose_estimation.PPFVoting in EdgePoints mode ("PPF EdgePoints mode") at PV1's sizes: a plate with holes
    # sampled by about 2 000 points, its edge points those detect_boundary_points finds on a dense sampling of the same plate; the
    # scene is the posed sample in 18 000 points of clutter (12 000 reference points at ratio 0.6), the scene's edges the posed
    # model edges and as many clutter edge points again.  Median of 5 calls after 1 warm-up for the table and the vote (once more
    # through device memory), of 3 for m3d_ppf_estimate_edges.  cpu_baseline = the contract's C restatement
    # (tests/cpp/ppf_ref.c with edge points) under OpenMP on 16 threads: the table whole, the vote on every tenth reference point, scaled.
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ppf_edge_ref_util as edge_util
    import ppf_ref_util as ppf_util

    pts, nrm, _, _, diameter = edge_util.plate_with_holes(n_side=57)
    dense, dense_n, _, _, _ = edge_util.plate_with_holes(n_side=130)
    eidx = capi.detect_boundary_points(dense, dense_n, capi.SEARCH_HYBRID, 0.03 * diameter, 30, 90.0).astype(np.int64)
    ept, enr = np.ascontiguousarray(dense[eidx]), np.ascontiguousarray(dense_n[eidx])
    r_min = 0.45 * diameter
    T = ppf_util.pose(1)
    sp, sn, _ = ppf_util.scene_of(pts, nrm, T, 20_000 - len(pts), 1)
    sep, sen, _ = ppf_util.scene_of(ept, enr, T, len(ept), 51)
    refs = np.sort(np.random.default_rng(1).permutation(len(sp))[: int(0.6 * len(sp))])

    ms_table, model = ppf_median(lambda: capi.PpfModel(pts, nrm, diameter, r_min, edge_points=ept, edge_normals=enr))
    ms_vote, (res, st) = ppf_median(lambda: model.vote(sp, sn, refs, stats=True, edge_points=sep, edge_normals=sen))
    capi.ppf_force(True, 0)
    try:
        ms_vote_dev, (res_dev, st_dev) = ppf_median(lambda: model.vote(sp, sn, refs, stats=True, edge_points=sep, edge_normals=sen))
    finally:
        capi.ppf_force(False, 0)
    ms_estimate, est = ppf_median(lambda: capi.ppf_estimate(model, sp, sn, refs, edge_points=sep, edge_normals=sen, score_thresh=0.0), 3)
    es = est["stats"]
    cpu_b = None
    if not NO_CPU:
        os.environ.setdefault("OMP_NUM_THREADS", "16")
        ref = ppf_util.PpfRef(tempfile.mkdtemp(), openmp=True)
        t0 = time.perf_counter()
        rm = ref.model(pts, nrm, diameter, r_min, edge_points=ept, edge_normals=enr)
        t1 = time.perf_counter()
        rv = rm.vote(sp, sn, refs[::10], sep, sen)
        t2 = time.perf_counter()
        cpu_b = {"ms_table": (t1 - t0) * 1e3, "ms_vote": (t2 - t1) * 1e3 * len(refs) / len(refs[::10]), "unit": "ms",
                 "vote_sampled": "every 10th reference point, scaled by the count", "increments_sampled": rv["increments"],
                 "same_table_size": bool(rm.n_entries == model.info()["n_entries"]),
                 "what": "tests/cpp/ppf_ref.c: the contract's restatement, gcc -O2 -ffp-contract=off -fopenmp, 16 threads"}
    emit("PV2 ppf EdgePoints: table of a plate with holes + vote and estimate on a 20 000-point scene, 12 000 reference points",
         n=len(pts), n_edge=len(ept), m=len(sp), m_edge=len(sep), n_ref=len(refs), table_entries=model.info()["n_entries"],
         ms_table=ms_table, ms_vote=ms_vote, ms_vote_device=st["ms_device"], path=st["path"], groups=st["groups"],
         launches=st["launches"], neighbours_visited=st["neighbours_visited"], increments=st["increments"], maxima=len(res["votes"]),
         increments_per_second=st["increments"] / (st["ms_device"] * 1e-3) if st["ms_device"] > 0 else None,
         device_memory_path={"ms_vote": ms_vote_dev, "ms_vote_device": st_dev["ms_device"], "path": st_dev["path"],
                             "same_result": bool(all(np.array_equal(res[k], res_dev[k]) for k in res))},
         estimate={"ms_total": ms_estimate, "ms_vote": es["ms_vote"], "ms_cluster": es["ms_cluster"], "ms_refine": es["ms_refine"],
                   "ms_host": es["ms_host"], "icp_calls": es["icp_calls"], "icp_iterations": es["icp_iterations"],
                   "results": len(est["votes"]), "top_votes": int(est["votes"][0]) if len(est["votes"]) else 0,
                   "top_score": float(est["scores"][0]) if len(est["votes"]) else 0.0,
                   "top_pose_error": float(np.abs(est["poses"][0] - T).max()) if len(est["votes"]) else None},
         roofline={"bound": "atomic increments (LDS or L2) and the divergent walk over table cells; no HBM or VALU ceiling is meaningful",
                   "share_of_peak": "not measured"},
         cpu_baseline=cpu_b)

if "PT1" in which or ALL:
    # pose_estimation.PPFEstimator.train ("PPF model preprocessing") on synth.box_surface_cloud at 1 M and at
    # 100 k points with the default config, normals estimated; m3d_ppf_prepare_model is also run with the dense sample, so that
    # the dense sampler and boundary detection are timed too (a closed box has no boundary: it finds no edge point).  One warm-up call, then the median of 3: the stages are m3d_ppf_model_info's own host clocks of that call.
    # cpu_baseline = the restatement (tests/cpp/ppf_train_ref.c, gcc -O2, one thread) on the normals the library's orientation was
    # given.  Its heap walk is timed APART from the brute-force neighbour lists it walks over (those are quadratic and no part of
    # the comparison) and from the samplers.  At 100 k it is run whole.  At 1 M the lists cannot be built: the walk's figure there is
    # SCALED from the 100 k run -- the walk is O(E log E) in the list entries E, and at a fixed radius E grows with n^2 (ten times
    # the points, each with ten times the neighbours), so ms_walk x 100 x log2(100 E) / log2(E); the samplers are not scaled.
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import misc3d_amd as m3d
    import ppf_train_ref_util as train_util

    walk_100k = None
    for n in (100_000, 1_000_000):
        pts, _ = synth.box_surface_cloud(n)
        runs = []
        for rep in range(4):
            t0 = time.perf_counter()
            r = capi.ppf_prepare_model(pts, None)
            runs.append(((time.perf_counter() - t0) * 1e3, r))
        ms_prepare, r = sorted(runs[1:], key=lambda x: x[0])[1]
        info, o = r["info"], r["info"]["orient"]
        est = m3d.pose_estimation.PPFEstimator(m3d.pose_estimation.PPFEstimatorConfig())
        train = []
        for rep in range(3):
            t0 = time.perf_counter()
            ok = est.train(pts)
            train.append((time.perf_counter() - t0) * 1e3)
        cpu_b = None
        if not NO_CPU and n <= 100_000:
            ref = train_util.TrainRef(tempfile.mkdtemp())
            nrm0 = capi.estimate_normals(pts, capi.SEARCH_HYBRID, info["normal_r"], 30)
            nrm0 = nrm0 / np.sqrt((nrm0[:, 0] * nrm0[:, 0] + nrm0[:, 1] * nrm0[:, 1]) + nrm0[:, 2] * nrm0[:, 2])[:, None]   # B3 (no zero normal here)
            if info["seed_flipped"]:
                nrm0[info["seed"]] = -nrm0[info["seed"]]                                                                   # B4
            on, _, ost, oms = ref.orient_timed(pts, nrm0, info["normal_r"], info["seed"])
            t0 = time.perf_counter()
            s_sparse = ref.sample(pts, info["dist_step"], info["seed"])
            t1 = time.perf_counter()
            ref.sample(pts, info["dist_step_dense"], info["seed"])
            t2 = time.perf_counter()
            walk_100k = (oms["ms_walk"], oms["list_entries"])
            cpu_b = {"ms_heap_walk": oms["ms_walk"], "list_entries": oms["list_entries"], "ms_brute_force_lists_not_compared": oms["ms_lists"],
                     "ms_sampler": (t1 - t0) * 1e3, "ms_dense_sampler": (t2 - t1) * 1e3, "unit": "ms",
                     "same_normals": bool(on.tobytes() == r["normals"].tobytes()), "same_stats": bool(all(ost[k] == o[k] for k in ost)),
                     "same_sample": bool(np.array_equal(s_sparse, r["sample_indices"])),
                     "what": "tests/cpp/ppf_train_ref.c, gcc -O2 -ffp-contract=off, one thread; the walk timed apart from its brute-force lists"}
        elif not NO_CPU and walk_100k:
            ms_w, e = walk_100k
            cpu_b = {"ms_heap_walk_scaled": ms_w * 100.0 * np.log2(100.0 * e) / np.log2(float(e)), "unit": "ms",
                     "scaled_from": "the 100 k run: ms_heap_walk x 100 (list entries grow with n^2 at a fixed radius) x log2(100 E) / log2(E)",
                     "ms_heap_walk_100k": ms_w, "list_entries_100k": e,
                     "what": "tests/cpp/ppf_train_ref.c's heap walk, not run at this size (its brute-force lists are quadratic)"}
        emit("PT1 ppf model preprocessing (with the dense sample) + PPFEstimator.train, synthetic box surface, default config", n=n,
             diameter=info["diameter"], normal_r=info["normal_r"], ms_prepare_model=ms_prepare, ms_box=info["ms_box"],
             ms_normals_and_orientation=info["ms_normals"],
             orientation={"ms_total": o["ms_total"], "ms_upload_and_grid": o["ms_grid"], "ms_rounds": o["ms_rounds"], "rounds": o["rounds"],
                          "ms_per_round": o["ms_rounds"] / max(o["rounds"], 1), "ms_tree_to_signs_host": o["ms_signs"],
                          "tree_edges": o["tree_edges"], "component": o["component"], "flips": o["flips"]},
             sampler={"ms": info["ms_sample"], "selected": len(r["sample_indices"]), "distance_evaluations": info["sample_distance_evaluations"]},
             dense_sampler={"ms": info["ms_dense"], "selected": len(r["dense_indices"]), "distance_evaluations": info["dense_distance_evaluations"]},
             boundary_detection={"ms": info["ms_edges"], "edges": len(r["edge_indices"])},
             train={"ok": bool(ok), "ms_median_of_3": sorted(train)[1], "ms_all": train, "model_sample": len(est.get_sampled_model()[0])},
             roofline={"bound": "the scan rounds re-read every 3x3x3 block once per round (latency- and L2-bound gathers of fp64 coordinates); not measured against a peak",
                       "share_of_peak": "not measured"},
             cpu_baseline=cpu_b)
