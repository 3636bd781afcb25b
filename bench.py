#!/usr/bin/env python
"""bench.py -- headline benchmark of the Misc3D RANSAC hot path on MI355X.

Metric (BASELINE.json): RANSAC hypotheses/sec (+ inlier-score GB/s) on a 1M-point cloud.
Workload at N = 1 (BASELINE.json configs[1], "C2"): fit_plane, 1 000 000 points, 10 000 hypotheses, threshold 0.01,
probability 1.0 (every hypothesis takes part), sampler seed 11.  A "step" is one complete FitModel: sample table ->
minimal fits -> scoring -> sequential best-model replay -> RefineModel (inlier list + least-squares plane) -> results
on the host.  The cloud is resident in HBM before the timed region (m3d_cloud_create).  `value` counts hypotheses
DISPOSED OF per second: every hypothesis' outcome in the reference's sequential loop is reproduced exactly, but only
the (512-point tile, hypothesis) pairs that can hold an inlier are evaluated point by point, and hypotheses whose
upper bound cannot reach an earlier hypothesis' count are pruned (both exact).

A plain run does what the headline needs: set-up (cloud, priming fits), W warm-up steps, K timed steps, the line.  `roofline`
(except `attainable`) is read from the timed steps themselves.  Every other object below takes runs of its own and is
measured only with --full.  --dump-outputs DIR writes the last timed step's results (params, inliers, summary = ret,
best_index, n_inliers, count, iterations) as float64 .npy files; the inputs are seeded, so two builds
can be compared output for output.

JSON objects besides the contract's fields:
  roofline     the bound that actually binds the dominant kernel score_screen_k<plane>: VALU issue.
               achieved = (tile, hypothesis) pairs the timed launches evaluated (counted inside the kernel,
               m3d_stats.pairs_timed) x 512 points x VALU instructions per (point, hypothesis) / the launches'
               duration measured live with HIP events on the library's stream (m3d_stats.ms_score_kernel) -- the
               same launches `rocprofv3 --kernel-trace --stats -- python bench.py` averages (profiles/).  One launch of
               this kernel per fit: the 128 leading hypotheses (3.5 % of the pairs) are counted inside cull_lead_k, the
               launch that also runs the box tests; neither their pairs nor its time are in this object.
               Instructions per (point, hypothesis): 3.625 for the plane's packed-fp32 screen (29 per lane and hypothesis for
               the lane's 8 points: 16 v_pk_fma, 8 v_alignbit, 4 v_min3, v_cmp -- the ISA of the loop, not an
               estimate; the fp64 loop it replaced: 7), 4.125 for the sphere (33 per 8 points in the expanded form; fp64: 10), 6.125 for the cylinder (49; fp64: 22).
               `frac` = the SIMD cycles the loop's instructions need at their MEASURED issue cost per class (peak_model:
               v_pk_fma_f32 4.20, v_alignbit 4.13, v_min3 4.15, v_cmp 4.21 cycles per wave instruction -- tools/ubench/valu_rates.hip,
               profiles/r04_ubench_valu_rates.txt; nothing in these loops issues in 2) over the cycles the launch had on 1024 SIMDs at 2.4 GHz;
               `peak` = the lane-instruction rate that corresponds to.  `traffic` = HBM bytes per launch from the committed PMC pass
               (`traffic_source`: counters cannot be collected inside a timed run).  `algorithmic_reuse` restates SURVEY.md 8(d)'s 24 B/(hypothesis, point) figure: it is far
               above the HBM peak because a point load is re-used from VGPRs by every hypothesis of a launch and most
               pairs are never touched -- not an HBM-bound kernel, so it is NOT the roofline.
  cpu_baseline the oracle's reference-shaped OpenMP port timed on this box's host cores (bounded sample), plus the
               same source built -O3 -march=native under "native".
  strong_scaling (N > 1) fixed TOTAL work, one-GPU time measured in the same job on rank 0: C2 (10 000 hypotheses)
               and C3 (cylinder / sphere, 1 M points, 50 000 hypotheses).

N > 1: `python bench.py --gpus N` starts N ranks itself (torch.distributed.run, one per GPU); under an external
launcher (WORLD_SIZE set) it is one of the ranks.  Control plane (rendezvous, barrier, max over ranks): torch.distributed
"gloo".  Data path: the C++ driver m3d_cloud_fit_sharded with a library-owned RCCL communicator (ncclAllGather of the
4-byte records on the library's stream over xGMI), ncclUniqueId handed out through the process group.
--scaling weak (the DEFAULT at every N: ONE headline workload, per-GPU work fixed, so that the driver can derive an efficiency
from the per-N values): --hyp hypotheses PER GPU of one stream, value = N x hyp / t.  `scaling: "weak"` in the line says so:
the per-N values are NOT the north_star's strong-scaling curve.  That question -- fixed TOTAL work -- is answered by the
`strong_scaling` block every N > 1 line carries with --full (C2, C3 cylinder, C3 sphere: one-GPU time measured in the same job, the
term-by-term model's prediction beside each), and what N GPUs deliver on independent jobs by the `replicas` block (no collective).
--scaling strong: --hyp hypotheses in total, value = hyp / t; with --full a `weak_scaling` block rides along instead.

More objects of the N = 1 line (--full):
  fp64_only    the same K steps with m3d_config.score_fp32_screen = 0, cull_fp32 = 0 (the reference's arithmetic only) and
               the VALU-issue fraction of score_mask_k on them: `value` read on the reference's own arithmetic.
  setup_ms     m3d_cloud_create (SetPointCloud's copy: upload, transpose, Hilbert sort, tile boxes), which the timed steps
               do NOT contain (cloud resident), with its phases.
  oneshot_ms   m3d_fit_plane from host arrays: create + fit + destroy per call, the reference's FitPlane shape.
  cpu_baseline.parity   the CPU port run on the GPU's own job (same cloud, same 10 000 hypotheses): best_index, count,
               the full inlier list and the refined parameters compared.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec
FP64_VALU_PEAK_TOPS = 39.3     # 256 CU x 4 SIMD x 16 fp64 lanes/clk x 2.4 GHz (non-FMA ops; FMA peak 78.6 TF): 4 cycles per wave instruction
# What a wave64 instruction of each class costs its SIMD, measured (tools/ubench/valu_rates.hip, 8 waves per SIMD, launch wall
# time at the sustained clock: profiles/r04_ubench_valu_rates.txt).  VERDICT r3 asked whether the plain fp32 / integer
# instructions issue in 2 cycles (MI355X_MICROARCH.md's v_fma_f32 row): they do not -- every VOP3-encoded instruction takes ~4.15,
# only 32-bit-encoded VOP2 integer / mul / add reach 2.3, and the scoring loops contain none of those.
CLASS_CYCLES = {"v_pk_fma_f32": 4.20, "v_pk_add_f32": 4.14, "v_alignbit_b32": 4.13, "v_min3_f32": 4.15, "v_cmp_f32": 4.21,
                "v_lshrrev_b32": 2.27, "v_mul_f32_e32": 2.31, "f64": 4.17, "v_cmp_f64": 4.19}
SIMDS, CLOCK_HZ = 1024, 2.4e9
# instructions per hypothesis and lane (8 points) of the loops, as the ISA has them (m3d_cull_kernels.hip, screen_eval / tile_count)
MIX_SCREEN = {0: {"v_pk_fma_f32": 16, "v_alignbit_b32": 8, "v_min3_f32": 4, "v_cmp_f32": 1},
              1: {"v_pk_fma_f32": 16, "v_pk_add_f32": 4, "v_alignbit_b32": 7, "v_min3_f32": 4, "v_cmp_f32": 1, "v_lshrrev_b32": 1},
              2: {"v_pk_fma_f32": 36, "v_alignbit_b32": 8, "v_min3_f32": 4, "v_cmp_f32": 1}}
MIX_FP64 = {0: {"f64": 48, "v_cmp_f64": 8}, 1: {"f64": 64, "v_cmp_f64": 16}, 2: {"f64": 160, "v_cmp_f64": 16}}


def peak_model(mix):
    """(instructions per 8 points, SIMD cycles per 8 points, the per-class table) of an instruction mix"""
    n = sum(mix.values())
    cyc = sum(k * CLASS_CYCLES[c] for c, k in mix.items())
    return n, cyc, {c: {"per_8_points": k, "cycles": CLASS_CYCLES[c]} for c, k in mix.items()}
ALG_BYTES_PER_PAIR = 24.0      # one fp64 xyz read per (hypothesis, point), SURVEY.md 8(d)
VALU_OPS_FP64 = {0: 7, 1: 10, 2: 22}      # fp64 VALU instructions per (point, hypothesis) incl. compares: score_mask_k, score_k
VALU_OPS_SCREEN = {0: 3.625, 1: 4.125, 2: 6.125}     # score_screen_k: packed-fp32 screen (m3d_cull_kernels.hip): 29 / 33 / 49 instructions per 8 points
KERNEL_FP64 = {0: "m3d::score_mask_k<0>", 1: "m3d::score_mask_k<1>", 2: "m3d::score_mask_k<2>"}
KERNEL_SCREEN = {0: "m3d::score_screen_k<0>", 1: "m3d::score_screen_k<1>", 2: "m3d::score_screen_k<2>"}
WORKLOADS = {   # name -> (kind, default hypotheses, threshold, seed, label)
    "c2": (0, 10_000, 0.01, 11, "C2 fit_plane"),
    "c3cyl": (2, 50_000, 0.01, 13, "C3 fit_cylinder"),
    "c3sph": (1, 50_000, 0.01, 13, "C3 fit_sphere"),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="c2")
    ap.add_argument("--hyp", type=int, default=0, help="hypotheses per step: per GPU (weak) or in total (strong); 0 = the workload's")
    ap.add_argument("--scaling", choices=("weak", "strong"), default=None,
                    help="default: weak (N x hyp hypotheses of one stream; the strong-scaling block rides along at N > 1)")
    ap.add_argument("--allow-host-transport", action="store_true",
                    help="N > 1: exit 0 even when the records went over gloo instead of RCCL (default: the line is printed, marked, rc 3)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-strong-extra", action="store_true", help="N > 1: skip the strong-scaling block")
    ap.add_argument("--kernel-detail", action="store_true",
                    help="extra stand-alone launches: fp64-VALU fraction on the unpruned launch, cull kernel, dense kernel")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline as well: cold, without_kernel_timing_events, fp64_only, plane_bound, "
                         "setup_ms, oneshot_ms, cpu_baseline, roofline.attainable; N > 1: strong_scaling, weak_scaling, replicas")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's results (params, inliers, summary) to DIR/<name>.npy as float64")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    return a


DUMP_MAX_ELEMENTS = 6_000_000      # 48 MB of float64: a longer inlier list is dumped as a fixed, seeded sample


def dump_outputs(d, res):
    """What a caller of the timed step receives (Cloud.fit: ret, params, inlier list, stats), as float64 arrays.  Indices
    and counts are exact in float64; of the stats only the integer results are kept (the timings differ from run to run,
    inlier_rmse is NaN on this path and fitness is n_inliers / N)."""
    os.makedirs(d, exist_ok=True)
    st = res.stats
    inl = np.asarray(res.inliers)
    if len(inl) > DUMP_MAX_ELEMENTS:
        inl = inl[np.sort(np.random.default_rng(0).choice(len(inl), DUMP_MAX_ELEMENTS, replace=False))]
    arrays = {"params": np.asarray(res.params, dtype=np.float64),
              "inliers": inl.astype(np.float64),
              "summary": np.array([res.ret, st["best_index"], st["n_inliers"], st["count"], st["iterations"]], dtype=np.float64)}
    for name, v in arrays.items():
        np.save(os.path.join(d, name + ".npy"), v)


def respawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: become the launcher."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),
               OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "8"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def load_pmc_traffic():
    """(HBM bytes per scoring launch, where the number comes from): the committed PMC pass profiles/pmc_score_latest.json --
    counters cannot be collected inside a timed run, so `roofline.traffic` is NOT measured by this process."""
    p = os.path.join(ROOT, "profiles", "pmc_score_latest.json")
    try:
        with open(p) as f:
            d = json.load(f)
        return d.get("hbm_bytes_per_launch"), {"file": "profiles/pmc_score_latest.json", "kernel": d.get("kernel"),
                                                "measured_at_commit": d.get("measured_at_commit"), "command": d.get("command"),
                                                "corrections": d.get("corrections")}
    except Exception:
        return None, None


def predicted_speedup(workload, world):
    """What the term-by-term model measured on ONE GPU (tools/model_strong_scaling.py: every rank's share of the sharded loop
    timed in turn + what every rank still does alone) predicts for `world` GPUs, exchange 30 / 60 us: the latest
    profiles/r*_strong_scaling_model.jsonl."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_strong_scaling_model.jsonl")))
    if not files:
        return None
    try:
        for line in open(files[-1]):
            d = json.loads(line)
            if d.get("workload") == workload and f"modelled_speedup_world{world}_exchange_30us" in d:
                return {"exchange_30us": d[f"modelled_speedup_world{world}_exchange_30us"],
                        "exchange_60us": d[f"modelled_speedup_world{world}_exchange_60us"], "source": os.path.relpath(files[-1], ROOT)}
    except Exception:   # noqa: BLE001
        pass
    return None


def usable_cpus():
    """CPUs this process may really use (oracle.usable_cpus: affinity mask capped by the cgroup quota).  The oracle is
    imported here, inside the cpu_baseline leg's helper, and nowhere else in this file."""
    import oracle
    return oracle.usable_cpus()


def cpu_baseline(pts, thr, seed, budget_s, H_gpu):
    """Reference-shaped OpenMP port (oracle/misc3d_oracle.c orc_fit_omp_baseline: omp parallel for over hypotheses,
    per-point virtual-dispatch-like distance with sqrt and divide, -O3 no -march like CMakeLists.txt:7,15-16) and the
    same source built -O3 -march=native.  The port's timed sample is the GPU's OWN workload -- the same cloud, exactly
    H_gpu hypotheses of the same sampler stream -- whenever that fits the budget (C2: ~2.5 s on 16 cores), so its result
    is directly comparable with the GPU's (`parity`); otherwise, and for the native build, a bounded prefix of it."""
    import oracle
    hw = usable_cpus()

    def run(fit_fn, set_threads, threads, H):
        set_threads(threads)
        t0 = time.perf_counter()
        model, cnt, bi = fit_fn(0, pts, None, thr, H, seed)
        dt = time.perf_counter() - t0
        return H / dt, H, dt, (model, cnt, bi)

    def calibrate(fit_fn, set_threads, threads):
        """seconds per hypothesis at this thread count: a short run to size a ~1 s one (a 30 ms probe picked the wrong
        count on a busy box)"""
        set_threads(threads)
        fit_fn(0, pts, None, thr, max(threads, 4), seed)                      # thread pool / page warm-up
        t0 = time.perf_counter()
        fit_fn(0, pts, None, thr, 2 * max(threads, 4), seed)
        per_h = (time.perf_counter() - t0) / (2 * max(threads, 4))
        H1 = int(max(2 * threads, min(4000, (budget_s / 12.0) / max(per_h, 1e-9))))
        H1 = (H1 // threads) * threads or threads
        t0 = time.perf_counter()
        fit_fn(0, pts, None, thr, H1, seed)
        return (time.perf_counter() - t0) / H1

    out, extra, out_res = None, None, None
    for kind_name, getter in (("port", lambda: (oracle.fit_omp_baseline, oracle.set_omp_threads)),
                              ("native", oracle.native_baseline)):
        try:
            fit_fn, set_threads = getter()
        except Exception as e:       # noqa: BLE001 -- the native build needs gcc on the box
            if kind_name == "native":
                extra = {"error": f"{type(e).__name__}: {e}"}
                continue
            raise
        cands = sorted({hw, max(1, hw // 2)})
        per_h = {t: calibrate(fit_fn, set_threads, t) for t in cands}
        best_t = min(per_h, key=per_h.get)
        share = budget_s * (0.6 if kind_name == "port" else 0.25)
        H = H_gpu if (kind_name == "port" and per_h[best_t] * H_gpu <= 1.5 * share) else int(
            max(best_t * 2, min(H_gpu, share / max(per_h[best_t], 1e-9))))
        if H != H_gpu:
            H = (H // best_t) * best_t or best_t
        rate, H, dt, res = run(fit_fn, set_threads, best_t, H)
        rec = {"value": rate, "unit": "hypotheses/s", "cores": best_t,
               "sample": f"fit_plane {len(pts)} pts x {H} hypotheses (thr {thr}, seed {seed}; the GPU's step has {H_gpu}), "
                         f"{dt:.1f} s, OpenMP static schedule over hypotheses; thread probe {{threads: hyp/s}} = "
                         + json.dumps({str(k): round(1.0 / v, 1) for k, v in per_h.items()}),
               "inlier_score_GBps": rate * len(pts) * ALG_BYTES_PER_PAIR / 1e9, "usable_cpus": hw}
        if kind_name == "port":
            rec["kind"] = "port"
            rec["flags"] = "-O3 -ffp-contract=off (no -march), as the reference's CMakeLists.txt"
            out, out_res = rec, res + (H,)
        else:
            rec["flags"] = "-O3 -march=native -ffp-contract=off"
            extra = rec
    out["native"] = extra
    return out, out_res


def make_cloud(workload, n, synth):
    kind = WORKLOADS[workload][0]
    if kind == 0:
        return synth.plane_cloud_c2(n, seed=2), None
    if kind == 1:
        return synth.sphere_cloud_c3(n, 4), None
    return synth.cylinder_cloud_c3(n, 3)


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(respawn_ranks(a.gpus))
    if a.scaling is None:
        # the headline is ONE workload at every N (the driver derives the scaling efficiency from the per-N values): BASELINE's
        # C2 with the per-GPU work fixed.  The north_star's fixed-total question is answered in the strong_scaling block of
        # every N > 1 line, for the workloads the term-by-term model says shard (C3 cylinder) and for those it says do not (C2).
        a.scaling = "weak"
    import torch
    import torch.distributed as dist
    from misc3d_amd import capi, synth

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # rehearsal of the N > 1 flow on a box with ONE GPU (tests/test_gpu_bench_multirank.py): every rank on device 0 and the
    # records over the process group through m3d_comm's host transport -- RCCL refuses two ranks on one device.  The
    # JSON line says so (config.parallelism); never a number to quote.
    rehearsal = os.environ.get("M3D_BENCH_REHEARSAL") == "1"
    if rehearsal:
        local = 0
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    comm = None
    transport_note = ""
    rccl_init_ms = None
    if world > 1:
        dist.init_process_group("gloo")                 # control plane only
        # data path: library-owned RCCL communicator (rehearsal: the caller-supplied all-gather over gloo).  Should RCCL
        # not come up on some rank -- or its first exchange fail -- EVERY rank falls back to the host transport (the same
        # shard loop and kernels, the records over gloo), and the JSON line says so: a slower number beats none
        fake_failure = os.environ.get("M3D_BENCH_FAKE_RCCL_FAILURE") == "1"   # (test hook: exercises the fallback)
        if rehearsal and not fake_failure:
            comm = capi.Comm.torch_host()
        else:
            ok, why = 1, ""
            t_init = time.perf_counter()
            try:
                if fake_failure:
                    raise RuntimeError("simulated (M3D_BENCH_FAKE_RCCL_FAILURE)")
                comm = capi.Comm.rccl(device=local)
            except Exception as e:   # noqa: BLE001
                comm, ok, why = None, 0, f"{type(e).__name__}: {e}"
            rccl_init_ms = (time.perf_counter() - t_init) * 1e3
            flag = torch.tensor([ok], dtype=torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag.item()) == 0:
                if comm is not None:
                    comm.close()
                comm = capi.Comm.torch_host()
                transport_note = "RCCL communicator unavailable (" + (why or "on another rank") + ")"
                print(f"[bench] rank {rank}: {transport_note}; records go over gloo", file=sys.stderr)
    elif os.environ.get("M3D_BENCH_FORCE_SHARDED") == "1":   # the N > 1 driver on one GPU (world-1 communicator)
        comm = capi.Comm.rccl(world=1, rank=0, device=local)
    n_gpus = world
    kind, H_default, thr, seed, label = WORKLOADS[a.workload]
    prob = 1.0
    N = a.points
    H = a.hyp or H_default
    H_total = H * world if a.scaling == "weak" else H
    pts, nrm = make_cloud(a.workload, N, synth)
    cloud = capi.Cloud(pts, nrm, device=local)
    # the roofline wants the dominant kernel's launches timed LIVE inside the timed steps: HIP events around every
    # scoring launch (m3d_config.kernel_timing; off by default in the library: four event commands per chunk)
    capi.set_config(kernel_timing=1)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    def step():
        if comm is None:
            return cloud.fit(kind, thr, H_total, prob, seed=seed, copy=False)
        # (rank 0 takes the inlier list, the other ranks the model only -- inliers == NULL: their compaction stays in HBM and
        #  nothing of it crosses their host links; every rank still ends with the same parameters and count)
        return cloud.fit_sharded(comm, kind, thr, H_total, prob, seed=seed, copy=False, want_inliers=(rank == 0))

    # set-up, before the W warm-up steps: the library allocates its per-device scratch lazily on the first fits, and
    # the GPU leaves its idle clocks only under load; a driver that asks for a very short warm-up would otherwise time both
    # (measured with --steps 20 --warmup 5, what a driver may ask for: 10 set-up fits leave the clocks on their way up --
    # 0.295 ms per step, the scoring launch 108-110 us; 100 and 400 give the steady state the default 200-step run sees -- 0.280 ms,
    # 100 us.  150 fits = 45 ms of set-up.)
    PRIMING_FITS = int(os.environ.get("M3D_BENCH_PRIMING", "150"))
    import gc
    gc.collect()          # here, not next to the timed region: a full collection idles the GPU for tens of milliseconds
    if world > 1 and not rehearsal and not transport_note:
        # the first exchange over the RCCL communicator, guarded: if it fails on any rank, all of them switch transports
        ok, why = 1, ""
        try:
            step()
        except Exception as e:   # noqa: BLE001
            ok, why = 0, f"{type(e).__name__}: {e}"
        flag = torch.tensor([ok], dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 0:
            comm._h = None                  # (the broken communicator is left alone: destroying it may hang too)
            comm = capi.Comm.torch_host()
            transport_note = "the first RCCL exchange failed (" + (why or "on another rank") + ")"
            print(f"[bench] rank {rank}: {transport_note}; records go over gloo", file=sys.stderr)
    # ---- `cold`: what a caller sees who has just created the cloud -- the first fit, then W warm-up and K timed steps with NO
    # priming in front of them (clocks on their way up, the lane's scratch allocated by the first fit).  Measured first, so that
    # nothing has warmed anything; the contract's steady-state value follows behind the priming fits.
    cold = None
    if a.full and world == 1 and comm is None:
        barrier()
        t0 = time.perf_counter()
        step()
        first_ms = (time.perf_counter() - t0) * 1e3
        for _ in range(a.warmup):
            step()
        barrier()
        gc.disable()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        barrier()
        dtc = time.perf_counter() - t0
        gc.enable()
        cold = {"first_fit_ms": first_ms, "ms_per_step": dtc / a.steps * 1e3, "value": H_total * a.steps / dtc, "steps": a.steps,
                "warmup": a.warmup,
                "note": "the same W + K steps BEFORE the priming fits (M3D_BENCH_PRIMING, default 150) that precede the contract's "
                        "timed region: the cloud's first fit (scratch allocation, tile frames), then steps on a GPU whose clocks "
                        "are still rising"}
    for _ in range(PRIMING_FITS):
        step()
    for _ in range(a.warmup):
        res = step()
    barrier()
    k_ms_sum, k_launches, k_pairs, k_exact, k_pairs_all = 0.0, 0, 0, 0, 0
    # the interpreter's cyclic collector stays out of the timed region (as timeit does): with torch imported a
    # full collection takes tens of milliseconds, ~100 steps' worth
    gc.disable()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        res = step()
        st = res.stats
        k_ms_sum += st["ms_score_kernel"]
        k_launches += st["score_launches"]
        k_pairs += st["pairs_timed"]       # the pairs of the launches behind ms_score_kernel (a lead pass inside cull_lead_k is not)
        k_pairs_all += st["pairs_scored"]
        k_exact += st["pairs_exact"]
    barrier()
    dt = time.perf_counter() - t0
    gc.enable()
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    ms_per_step = dt / a.steps * 1e3
    value = H_total * a.steps / dt
    coll_per_step = comm.collectives / float(PRIMING_FITS + a.warmup + a.steps) if comm is not None else 0.0
    # here, before any further fit: res.inliers is a view of the cloud's output buffer (copy=False), which the next fit overwrites
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, res)
    # the same steps as a caller gets them (no timing events in the stream): reported beside the contract's number
    dt_plain = None
    if a.full:
        capi.set_config(kernel_timing=0)
        for _ in range(5):
            step()
        barrier()
        gc.disable()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        barrier()
        dt_plain = time.perf_counter() - t0
        gc.enable()
        if world > 1:
            t = torch.tensor([dt_plain], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt_plain = float(t.item())
        capi.set_config(kernel_timing=1)

    # ---- N = 1: the same steps on the reference's own arithmetic, the set-up the timed steps do not contain, and the
    # reference-shaped call (host arrays in, results out: py_common.cpp:11-27 has no resident handle) ----------------
    fp64_only, setup, oneshot, plane_bound = None, None, None, None
    if a.full and world == 1 and comm is None:
        old_cfg = capi.set_config(score_fp32_screen=0, cull_fp32=0)
        try:
            for _ in range(5):
                step()
            barrier()
            f_ms, f_launch, f_pairs = 0.0, 0, 0
            gc.disable()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                r64 = step()
                f_ms += r64.stats["ms_score_kernel"]
                f_launch += r64.stats["score_launches"]
                f_pairs += r64.stats["pairs_timed"]
            barrier()
            dt64 = time.perf_counter() - t0
            gc.enable()
            same64 = (r64.stats["best_index"] == res.stats["best_index"] and np.array_equal(r64.inliers, res.inliers)
                      and np.array_equal(r64.params, res.params))
            v64 = f_pairs * 512.0 * VALU_OPS_FP64[kind] / (f_ms * 1e-3) / 1e12
            fp64_only = {"ms_per_step": dt64 / a.steps * 1e3, "value": H_total * a.steps / dt64,
                         "config": "m3d_config.score_fp32_screen = 0, cull_fp32 = 0: box tests and point tests in fp64 only, the "
                                   "reference's arithmetic instruction for instruction (score_mask_k, cull_tiles_k)",
                         "identical_result": bool(same64),
                         "roofline": {"bound": "valu-issue", "kernel": KERNEL_FP64[kind], "achieved": v64,
                                      "peak": SIMDS * 64.0 * CLOCK_HZ / (peak_model(MIX_FP64[kind])[1] / peak_model(MIX_FP64[kind])[0]) / 1e12,
                                      "frac": f_pairs * peak_model(MIX_FP64[kind])[1] / (f_ms * 1e-3 * SIMDS * CLOCK_HZ),
                                      "ops_per_pair": VALU_OPS_FP64[kind], "launch_ms": f_ms / max(f_launch, 1),
                                      "launches_per_step": f_launch / float(a.steps),
                                      "tile_hypothesis_pairs_per_step": f_pairs / float(a.steps)}}
        finally:
            capi.restore_config(old_cfg)
        # the planes' histogram bound (m3d_bound.hip) switched off: the same K steps, same result, what the bound is worth
        if kind == 0 and capi.get_config().plane_bound != 0:
            old_cfg = capi.set_config(plane_bound=0)
            try:
                for _ in range(5):
                    step()
                barrier()
                b_ms, b_launch, b_pairs = 0.0, 0, 0
                gc.disable()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    rb = step()
                    b_ms += rb.stats["ms_score_kernel"]
                    b_launch += rb.stats["score_launches"]
                    b_pairs += rb.stats["pairs_timed"]
                barrier()
                dtb = time.perf_counter() - t0
                gc.enable()
                sameb = (rb.stats["best_index"] == res.stats["best_index"] and np.array_equal(rb.inliers, res.inliers)
                         and np.array_equal(rb.params, res.params))
                plane_bound = {"without": {"ms_per_step": dtb / a.steps * 1e3, "value": H_total * a.steps / dtb,
                                           "launch_ms": b_ms / max(b_launch, 1),
                                           "tile_hypothesis_pairs_per_launch": b_pairs / max(b_launch, 1),
                                           "frac": b_pairs * peak_model(MIX_SCREEN[kind])[1] / (b_ms * 1e-3 * SIMDS * CLOCK_HZ),
                                           "identical_result": bool(sameb)},
                               "note": "m3d_config.plane_bound = 0: the keep rule prices a hypothesis at 512 points per tile its slab "
                                       "can touch; with the bound (the headline) at a per-tile histogram's mass over the slab "
                                       "(tile_frames_k once per resident cloud, plane_bound_k per fit: inside ms_per_step)"}
            finally:
                capi.restore_config(old_cfg)
            # what the first long plane fit of a cloud pays for the tile frames (one launch of tile_frames_k)
            capi.set_config(kernel_timing=0)
            first, second = [], []
            for i in range(4):
                c_tmp = capi.Cloud(pts, nrm, device=local)
                c_tmp._out_buf()   # (the wrapper's page-locked index-list buffer: 8 MB of hipHostMalloc, not the library's business)
                barrier()
                t0 = time.perf_counter(); c_tmp.fit(kind, thr, H_total, prob, seed=seed, copy=False); barrier()
                t1 = time.perf_counter(); c_tmp.fit(kind, thr, H_total, prob, seed=seed, copy=False); barrier()
                t2 = time.perf_counter()
                if i:
                    first.append((t1 - t0) * 1e3)
                    second.append((t2 - t1) * 1e3)
                c_tmp.close()
            capi.set_config(kernel_timing=1)
            plane_bound["first_fit_of_a_cloud_ms"] = float(np.mean(first))
            plane_bound["second_fit_ms"] = float(np.mean(second))
        # set-up: m3d_cloud_create = SetPointCloud's copy (ransac.h:469-475) -- upload, transpose, Hilbert sort, tile boxes
        capi.set_config(kernel_timing=0)
        tot = []
        for i in range(6):
            c_tmp = capi.Cloud(pts, nrm, device=local)
            if i:
                tot.append(c_tmp.setup_ms()["total"])
            c_tmp.close()
        capi.set_config(kernel_timing=1)
        ph = []
        for i in range(4):
            c_tmp = capi.Cloud(pts, nrm, device=local)
            if i:
                ph.append(c_tmp.setup_ms())
            c_tmp.close()
        setup = {"ms": float(np.mean(tot)), "ms_min": float(np.min(tot)),
                 "phases_ms": {k: float(np.mean([q[k] for q in ph])) for k in ph[0] if k != "total"},
                 "bytes_uploaded": int(pts.nbytes + (nrm.nbytes if nrm is not None else 0)),
                 "note": "m3d_cloud_create from the caller's pageable numpy array, not inside `value` (SURVEY.md 8(d): cloud "
                         "resident, upload reported separately); phases measured in separate creations with a stream "
                         "synchronisation after each phase"}
        # one-shot: m3d_fit_plane(xyz, n, ...) -- create + fit + destroy per call, what a drop-in FitPlane caller pays
        capi.set_config(kernel_timing=0)
        for _ in range(3):
            capi.fit(kind, pts, nrm, thr, H_total, prob, seed=seed, copy=False)
        barrier()
        one = []
        for _ in range(10):
            t0 = time.perf_counter()
            r1 = capi.fit(kind, pts, nrm, thr, H_total, prob, seed=seed, copy=False)
            one.append((time.perf_counter() - t0) * 1e3)
        same1 = (r1.stats["best_index"] == res.stats["best_index"] and np.array_equal(r1.inliers, res.inliers)
                 and np.array_equal(r1.params, res.params))
        oneshot = {"ms": float(np.mean(one)), "ms_min": float(np.min(one)), "value": H_total / (float(np.mean(one)) * 1e-3),
                   "identical_result": bool(same1),
                   "call": "m3d_fit_plane / _sphere / _cylinder from host arrays (pageable numpy in, parameters + index list "
                           "out), the shape of the reference's FitPlane (python/py_common.cpp:11-27)"}
        capi.set_config(kernel_timing=1)

    # ---- N > 1: strong scaling at fixed total work, one-GPU time measured in the same job (rank 0 alone) ----------
    strong = None
    if a.full and world > 1 and not a.no_strong_extra:
        strong = {}
        for wl in ("c2", "c3cyl", "c3sph"):
            k2, h2, thr2, seed2, label2 = WORKLOADS[wl]
            if wl == a.workload:
                c2 = cloud
            else:
                p2, n2 = make_cloud(wl, N, synth)
                c2 = capi.Cloud(p2, n2, device=local)
            reps = 20 if wl == "c2" else 6
            for _ in range(3):
                c2.fit_sharded(comm, k2, thr2, h2, 1.0, seed=seed2, copy=False, want_inliers=(rank == 0))
            barrier()
            t0 = time.perf_counter()
            for _ in range(reps):
                rs = c2.fit_sharded(comm, k2, thr2, h2, 1.0, seed=seed2, copy=False, want_inliers=(rank == 0))
            barrier()
            tn = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
            dist.all_reduce(tn, op=dist.ReduceOp.MAX)
            t1 = None
            if rank == 0:
                for _ in range(3):
                    r1 = c2.fit(k2, thr2, h2, 1.0, seed=seed2, copy=False)
                t0 = time.perf_counter()
                for _ in range(reps):
                    r1 = c2.fit(k2, thr2, h2, 1.0, seed=seed2, copy=False)
                t1 = (time.perf_counter() - t0) / reps * 1e3
                same = (r1.stats["best_index"] == rs.stats["best_index"] and r1.stats["n_inliers"] == rs.stats["n_inliers"]
                        and np.array_equal(r1.params, rs.params))
                strong[wl] = {"workload": f"{label2}, {N} pts, {h2} hypotheses in total", "ms_1gpu": t1,
                              "model_predicted_speedup": predicted_speedup(wl, world),
                              f"ms_{world}gpu": float(tn.item()) / reps * 1e3,
                              "speedup": t1 / (float(tn.item()) / reps * 1e3), "identical_to_1gpu": bool(same),
                              "best_index": int(rs.stats["best_index"]), "n_inliers": int(rs.stats["n_inliers"])}
            barrier()
            if c2 is not cloud:
                c2.close()

    # ---- N > 1 with the strong headline: the weak-scaling number rides along (N x hyp hypotheses of one stream) ---------
    weak = None
    if a.full and world > 1 and a.scaling == "strong" and not a.no_strong_extra:
        Hw = H * world
        for _ in range(3):
            cloud.fit_sharded(comm, kind, thr, Hw, prob, seed=seed, copy=False, want_inliers=(rank == 0))
        barrier()
        t0 = time.perf_counter()
        for _ in range(20):
            cloud.fit_sharded(comm, kind, thr, Hw, prob, seed=seed, copy=False, want_inliers=(rank == 0))
        barrier()
        tw = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
        dist.all_reduce(tw, op=dist.ReduceOp.MAX)
        weak = {"workload": f"{label}, {N} pts, {H} hypotheses per GPU ({Hw} in total)", "ms_per_step": float(tw.item()) / 20 * 1e3,
                "value": Hw * 20 / float(tw.item()), "unit": "hypotheses/s"}

    # ---- N > 1: what N GPUs deliver on INDEPENDENT fits (replicas: every rank fits its own job on its own GPU, no collective,
    # no replicated sampler / MinimalFit / RefineModel beyond its own) -- the throughput figure next to the one-stream numbers
    replicas = None
    if a.full and world > 1:
        for _ in range(3):
            cloud.fit(kind, thr, H, prob, seed=seed + rank, copy=False)
        barrier()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            cloud.fit(kind, thr, H, prob, seed=seed + rank, copy=False)
        barrier()
        tr = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
        dist.all_reduce(tr, op=dist.ReduceOp.MAX)
        replicas = {"workload": f"{label}: {world} independent fits in flight, one per rank ({H} hypotheses each, sampler seed + rank)",
                    "ms_per_step": float(tr.item()) / a.steps * 1e3, "value": H * world * a.steps / float(tr.item()),
                    "unit": "hypotheses/s", "collectives": 0,
                    "note": "not the headline: `value` above is ONE hypothesis stream sharded over the ranks"}

    transports = None
    if world > 1:
        mine = {"rank": rank, "device": local,
                "transport": ("gloo all-gather over host memory: " + transport_note if transport_note else
                              ("gloo all-gather over host memory (rehearsal)" if rehearsal else "RCCL ncclAllGather on the library's stream")),
                "rccl_init_ms": rccl_init_ms}
        transports = [None] * world
        dist.all_gather_object(transports, mine)
    if rank == 0:
        n_in = len(res.inliers)
        n_tiles = -(-N // 512)
        traffic, traffic_source = load_pmc_traffic() if a.workload == "c2" else (None, None)
        k_ms = k_ms_sum / max(k_launches, 1)
        h_rank = H_total / world                                  # hypotheses this rank scores per step
        h_per_launch = h_rank * a.steps / max(k_launches, 1)
        screened = bool(capi.get_config().score_fp32_screen)
        ops = (VALU_OPS_SCREEN if screened else VALU_OPS_FP64)[kind]
        kname = (KERNEL_SCREEN if screened else KERNEL_FP64)[kind]
        v_tops = k_pairs * 512.0 * ops / (k_ms_sum * 1e-3) / 1e12
        alg_bytes = h_per_launch * float(N) * ALG_BYTES_PER_PAIR
        alg_rate = alg_bytes / (k_ms * 1e-3) / 1e9
        # the peak is priced per instruction class: a (tile, hypothesis) pair costs its wave the loop's
        # instruction mix once; the SIMD cycles that takes at the measured issue costs, over the cycles the launch had
        n_mix, cyc_mix, mix_table = peak_model((MIX_SCREEN if screened else MIX_FP64)[kind])
        peak_tops = SIMDS * 64.0 * CLOCK_HZ / (cyc_mix / n_mix) / 1e12
        frac = k_pairs * cyc_mix / (k_ms_sum * 1e-3 * SIMDS * CLOCK_HZ)
        roofline = {"bound": "valu-issue", "kernel": kname, "achieved": v_tops, "peak": peak_tops,
                    "unit": "T lane-instructions/s (VALU issue)", "frac": frac,
                    "peak_model": {"instructions_per_8_points": n_mix, "simd_cycles_per_8_points": cyc_mix, "classes": mix_table,
                                   "simds": SIMDS, "clock_hz": CLOCK_HZ,
                                   "source": "profiles/r04_ubench_valu_rates.txt (tools/ubench/valu_rates.hip: cycles per wave "
                                             "instruction per SIMD, 8 waves per SIMD, at the sustained clock)",
                                   "frac_if_every_instruction_took_4_cycles": v_tops / FP64_VALU_PEAK_TOPS},
                    "traffic": traffic, "traffic_source": traffic_source, "launch_ms": k_ms, "launches_timed": k_launches,
                    "hypotheses_per_launch": h_per_launch, "ops_per_pair": ops,
                    "arithmetic": ("packed fp32 screen with a rounding bound (v_pk_fma_f32), exact fp64 recount of the undecided pairs"
                                   if screened else "fp64"),
                    "pairs_recounted_in_fp64_fraction": k_exact / max(k_pairs_all, 1),
                    "tile_hypothesis_pairs_per_launch": k_pairs / max(k_launches, 1),
                    "pairs_evaluated_fraction": k_pairs_all / float(n_tiles * h_rank * a.steps),
                    "pairs_outside_the_timed_launches": (k_pairs_all - k_pairs) / max(k_launches, 1),
                    "timing": "HIP events attached to every launch of this kernel inside the timed steps (hipExtLaunchKernel start / stop events on the "
                              "library's stream, rank 0).  The 128 leading hypotheses of a fit are counted inside cull_lead_k, the launch that also "
                              "runs the box tests: their pairs (pairs_outside_the_timed_launches) and its time are not in this object",
                    "step_composition": {
                        "note": "with the histogram bound the scoring launch is no longer the longest kernel of a C2 step: "
                                "compact_write_k<0,0> (RefineModel's index list, ransac.h:537-543: n_inliers x 8 bytes written straight "
                                "into the caller's page-locked buffer) takes ~79 us at the host link's rate; the roofline object "
                                "stays on the scoring kernel -- the EvaluateModel loop (ransac.h:626-654) is the path's arithmetic",
                        "host_link": {"kernel": "m3d::compact_write_k<0, 0>", "bytes_per_step": int(n_in) * 8,
                                      "duration_us": 79.0, "duration_source": "profiles/ (rocprofv3 kernel stats of this command)",
                                      "rate_GBps": int(n_in) * 8 / 79.0e-6 / 1e9, "peak_GBps": 63.0,
                                      "peak_source": "PCIe 5.0 x16, one direction: 32 GT/s x 16 lanes x 128/130 / 8"}},
                    "algorithmic_reuse": {
                        "bytes_per_launch": alg_bytes, "rate_GBps": alg_rate, "x_hbm_peak": alg_rate / HBM_PEAK_GBS,
                        "inlier_score_GBps_whole_step": H_total * float(N) * ALG_BYTES_PER_PAIR * a.steps / dt / 1e9,
                        "hypotheses": "disposed of: scored, or pruned by a bound that proves they cannot win (their records are then 0)",
                        "note": "24 B x hypotheses x points of a launch / launch time (what EvaluateModel streams on the "
                                "CPU).  Exceeds the HBM peak BY CONSTRUCTION: each point load is re-used from VGPRs by "
                                "all hypotheses of the launch, box-culled (tile, hypothesis) pairs and pruned hypotheses "
                                "are never evaluated.  Reported for SURVEY.md 8(d); it is not a roofline fraction."}}
        if a.full:
            try:
                # what the chip SUSTAINS on independent fp64 mul / add chains (it clocks below 2.4 GHz under that load):
                # the attainable counterpart of `peak`, measured here, after the timed steps
                att, att_ms = capi.fp64_issue_rate(local, 3.0)
                roofline["attainable"] = {"peak_measured": att, "unit": roofline["unit"], "frac_of_measured_peak": v_tops / att,
                                          "probe": f"m3d_bench_fp64_issue_rate: 2048 workgroups x 256 threads of independent v_mul_f64 / "
                                                   f"v_add_f64 chains for {att_ms:.2f} ms; `frac` above stays quoted on the nominal peak"}
            except Exception as e:      # noqa: BLE001 -- a probe, never fatal
                roofline["attainable"] = {"error": str(e)}
        if a.kernel_detail:
            Hk = min(H, 16384)
            samples = capi.draw_samples(N, kind, Hk, seed)
            cloud.time_score(kind, thr, samples, reps=3, mode=0)            # clocks up
            u_ms, listed = cloud.time_score(kind, thr, samples, reps=10, mode=0)   # score_mask_k, nothing pruned
            cull_ms, _ = cloud.time_score(kind, thr, samples, reps=10, mode=1)      # cull_mask_k
            dense_ms, _ = cloud.time_score(kind, thr, samples, reps=5, mode=2)      # score_k: the unculled kernel
            valu_tops = listed * 512.0 * ops / (u_ms * 1e-3) / 1e12
            dense_tops = float(-(-Hk // 64) * 64) * float(-(-N // 2048) * 2048) * VALU_OPS_FP64[kind] / (
                dense_ms * 1e-3) / 1e12
            roofline["unpruned_launch"] = {"achieved": valu_tops, "peak": FP64_VALU_PEAK_TOPS,
                                           "frac": valu_tops / FP64_VALU_PEAK_TOPS, "launch_ms": u_ms, "hypotheses": Hk,
                                           "surviving_tile_hypothesis_pairs": listed,
                                           "surviving_fraction": listed / float(n_tiles * Hk)}
            roofline["cull_kernel_ms"] = cull_ms
            roofline["dense_kernel"] = {"kernel": f"m3d::score_k<{kind}>", "launch_ms": dense_ms,
                                        "frac": dense_tops / FP64_VALU_PEAK_TOPS}
        out = {"metric": "RANSAC hypotheses/sec, 1M-pt cloud (inlier-score GB/s: roofline.algorithmic_reuse)",
               "value": value, "unit": "hypotheses/s",
               "n_gpus": n_gpus, "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms_per_step,
               "higher_is_better": True, "scaling": (a.scaling if world > 1 else "none"), "vs_baseline": None,
               "dtype": ("f64 decisions (fp32 screen + fp64 recount)" if screened else "f64"),
               "data": "synthetic",
               "config": {"workload": label, "points": N, "hypotheses_per_gpu": H_total / world,
                          "hypotheses_total": H_total, "threshold": thr, "probability": prob, "sampler_seed": seed,
                          "parallelism": (f"hypothesis-sharded x{world}, C++ driver + " + ("gloo all-gather, ALL RANKS ON ONE GPU (rehearsal)"
                                                                                       if rehearsal else ("gloo all-gather over host memory -- " + transport_note if transport_note else "RCCL all-gather")) if world > 1 else
                                          ("single GPU through the sharded driver (world-1 RCCL communicator)" if comm
                                           else "single GPU")),
                          "setup_fits_before_warmup": PRIMING_FITS},
               "result": {"best_index": int(res.stats["best_index"]), "n_inliers": int(n_in),
                          "params": [float(v) for v in res.params]},
               "roofline": roofline,
               "timing_breakdown_ms": {k: res.stats[k] for k in ("ms_sample", "ms_score", "ms_refine", "ms_total")}}
        if dt_plain is not None:
            out["without_kernel_timing_events"] = {"ms_per_step": dt_plain / a.steps * 1e3, "value": H_total * a.steps / dt_plain,
                                                   "note": "the same K steps again with m3d_config.kernel_timing = 0, the library's "
                                                           "default: `value` above carries the four HIP-event commands per chunk "
                                                           "that `roofline.launch_ms` is measured with"}
        if fp64_only:
            out["fp64_only"] = fp64_only
        if cold:
            out["cold"] = cold
        if plane_bound:
            out["plane_bound"] = plane_bound
        if setup:
            out["setup_ms"] = setup
        if oneshot:
            out["oneshot_ms"] = oneshot
        if comm is not None:
            out["collectives_per_step"] = coll_per_step
        if strong:
            out["strong_scaling"] = strong
        if weak:
            out["weak_scaling"] = weak
        if replicas:
            out["replicas"] = replicas
        if world > 1:
            out["transport"] = {"per_rank": transports,
                                "valid_headline": bool(not transport_note),
                                "note": "a line whose records went over gloo because RCCL did not come up is printed for diagnosis and the "
                                        "process exits 3 (--allow-host-transport: 0): it is not the RCCL number"}
            out["c5_note"] = ("iterative_plane_segmentation (BASELINE configs[4], 8 GPUs): sharding each round's 100-1000 hypotheses is "
                              "supported and bit-identical to one GPU (m3d_segment_plane_iterative_sharded) but not faster -- a round is "
                              "~80 us of latency-bound launches and compaction on a cloud that fits one GPU 1000 times over, a collective "
                              "per round costs what an eighth of the scoring saves (DESIGN.md 5).  What N GPUs are good for on this path "
                              "is N independent scenes in flight: m3d_segment_plane_iterative per device, tools/time_c5_plain.py "
                              "--devices N (replicas, no collective)")
        if a.full and world == 1 and not a.no_cpu_baseline and a.workload == "c2":
            import oracle
            cb, (cmodel, ccnt, cbi, ch) = cpu_baseline(pts, thr, seed, a.cpu_seconds, H_total)
            out["cpu_baseline"] = cb
            out["speedup_vs_cpu_baseline"] = value / cb["value"]
            # parity of the step just timed with the CPU run of the SAME job (same cloud, same H hypotheses of the same
            # stream): best hypothesis, its inlier count, and -- RefineModel of the CPU's best model, oracle.refine --
            # the full inlier index list and the refined parameters
            if ch == H_total:
                _ok, cpar, cinl = oracle.refine(kind, pts, thr, cmodel)
                out["cpu_baseline"]["parity"] = {
                    "best_index": bool(cbi == int(res.stats["best_index"])),
                    "count": bool(int(ccnt) == int(n_in)),
                    "inliers_equal": bool(np.array_equal(cinl, np.asarray(res.inliers))),
                    "params_max_abs_diff": float(np.max(np.abs(cpar - res.params))),
                    "cpu": {"best_index": int(cbi), "count": int(ccnt)},
                    "gpu": {"best_index": int(res.stats["best_index"]), "count": int(n_in)}}
            else:   # the CPU could not afford the whole job inside the budget: one record of its prefix instead
                s2 = capi.draw_samples(N, kind, ch, seed)
                _, _, c2 = cloud.score_range(kind, thr, s2, cbi, cbi + 1)
                out["cpu_baseline"]["parity"] = {"prefix_only": True, "hypotheses": int(ch),
                                                 "count_of_cpu_best": bool(int(c2[0]) == int(ccnt))}
        print(json.dumps(out), flush=True)
    barrier()
    cloud.close()
    if comm is not None:
        comm.close()
    if world > 1:
        dist.destroy_process_group()
        strict = os.environ.get("M3D_BENCH_STRICT") == "1"   # (test hook: the rule below on a one-GPU rehearsal)
        if transport_note and (not rehearsal or strict) and not a.allow_host_transport:
            sys.exit(3)   # (every rank: the launcher reports the failure)


if __name__ == "__main__":
    main()
