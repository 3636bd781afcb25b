"""No result may depend on what a recycled block of device scratch holds.

DevBuf::reserve hands out a fresh allocation or a block of the lane's free list with the last call's contents in it, so what
a kernel finds in a word nobody wrote in this call depends on the history of the process -- and in this suite that history
is an identical call, the most forgiving garbage there is.  m3d_bench_scratch_fill (include/misc3d_amd_bench.h) sets every
block to one byte as it is handed out; here every entry point that takes pooled blocks runs once with the hook off (the
baseline, which the entry point's own suite holds to its reference on these inputs) and once under each of

    0x00   a kernel that NEEDS zeros passes here and only here: what shows that the next three can fail
    0xFF   the largest index as uint32, a NaN as a double
    0x3F   about 4.8e-4 as a double: a finite, plausible summand no NaN check catches
    0x55   a large finite double, a large odd count

and every output array must be equal byte for byte, every integer statistic equal (timings excluded, and the one work counter
that is no function of the input: ORDER_DEPENDENT below).  A second leg runs a
small case, a sibling several times its size and the small case again on one thread (scratch that lives in the lane and only
grows is never handed out again, so the hook does not reach it), a third runs two threads under a fill.

Index-typed scratch, launch that writes each word -> launch that reads it ("Scratch contents", has the whole
list; read before the first filled run, since a filled block turns a stale index into a wild address):
  CellSort cell / rank     grid_count_k writes all n (0xFFFFFFFF for a point outside the grid) -> grid_scatter_k reads all n
  CellSort start[ncell+1]  memset to 0 before grid_count_k, scanned in place; [ncell] = the total, written by the scan
  CellSort sums / total    written by the scan's first pass for every tile -> read by its second
  k-NN / FPFH / normals    neighbour slots [0, count) written by the search, count written for every query -> readers stop at count
  proximity parent / label every row written by the init launch before the first hook launch reads it
  radius_neighbors offsets host prefix sum over device counts written for all n
  voxel keys / order / seg radix passes write all n of the ping-pong buffers; heads flagged for all n, scanned, then compacted
  PPF cell_offsets / nbr   counted from a memset, scanned, filled; the vote's accumulators are cleared per reference point
  PPF cluster label / adj  every row written by the pair kernels for n_valid rows; readers are bounded by n_valid
  registration validation  partial[tile][s] written for every tile of a phase and every s < s_pad; n_pairs cleared before redo_pairs_k
  ICP nn[i]                written for every i < n in every iteration (0xFFFFFFFF: none) before the sums gather through it
  raycast parent / visit   every node but the root named once by rc_tree_k; visit cleared per frame
"""
import struct
import threading

import numpy as np
import pytest

from misc3d_amd import synth

pytestmark = pytest.mark.gpu

PATTERNS = (0x00, 0xFF, 0x3F, 0x55)
PROBE_BYTES = 3 * (1 << 20) + 4096 + 8


@pytest.fixture(scope="module", autouse=True)
def _hook_off_afterwards(capi):
    yield
    capi.lib().m3d_bench_scratch_fill(-1)
    capi._scratch_pattern = -1


# ---- results as comparable records ------------------------------------------------------------------------------------------
# Work counters that are no function of the input.  grid_count_k ranks the points of a cell by the value an atomicAdd returns, so
# the order of the points INSIDE a cell of a counting-sorted copy -- and with it which points share a tile where a cell straddles
# a tile's end -- is the order the atomics landed in (tests/test_gpu_registration.py says the same of the registration's source
# copy).  Results do not depend on it; these counters of work done on tiles do, and are compared nowhere:
#   m3d_fps_stats.tiles_updated (+ the fraction derived from it): MEASURED -- two unfilled runs of the 8193-point case, back to
#     back, 0.5355 against 0.5359 pruned, the 64 sampled indices equal;
#   m3d_stats.pairs_scored / pairs_exact / pairs_timed: (tile, hypothesis) pairs that survive the box tests of the Hilbert-sorted copy;
#   m3d_reg_stats.lds_wave_hypotheses / global_wave_hypotheses / nn_screen_fallbacks: (source tile, hypothesis) pairs the candidate
#     cache certified or walked, queries the fp32 screen passed on -- equal in every run made so far, left out for the mechanism.
ORDER_DEPENDENT = ("tiles_updated", "pruned_fraction", "pairs_scored", "pairs_exact", "pairs_timed", "lds_wave_hypotheses",
                   "global_wave_hypotheses", "nn_screen_fallbacks")


def _left_out(key):
    return key == "ms" or key.startswith("ms_") or key.endswith("_ms") or key in ORDER_DEPENDENT


def _freeze(x, path="", out=None):
    """a result of any shape -> {path: bytes of an array | bytes of a double | int | None}, timings left out"""
    out = {} if out is None else out
    if isinstance(x, dict):
        for k in sorted(x):
            if not _left_out(str(k)):
                _freeze(x[k], f"{path}.{k}", out)
    elif isinstance(x, (list, tuple)):
        out[path + ".len"] = len(x)
        for i, v in enumerate(x):
            _freeze(v, f"{path}[{i}]", out)
    elif isinstance(x, np.ndarray):
        out[path] = (x.dtype.str, x.shape, np.ascontiguousarray(x).tobytes())
    elif isinstance(x, (bool, int, np.integer, np.bool_)):
        out[path] = int(x)
    elif isinstance(x, (float, np.floating)):
        out[path] = struct.pack("<d", float(x))
    elif x is None:
        out[path] = None
    elif hasattr(x, "params") and hasattr(x, "inliers"):      # capi.Fit
        _freeze(dict(ret=x.ret, params=x.params, inliers=x.inliers, stats=x.stats), path, out)
    else:
        raise TypeError(f"{path}: {type(x)}")
    return out


def _differences(a, b):
    return sorted(k for k in set(a) | set(b) if k not in a or k not in b or a[k] != b[k])


# ---- the panel: name -> builder(capi, big) -> run().  A builder makes the inputs (hook off); run() makes every device call
# of the case, the persistent objects (k-NN index, PPF model) included, so that they too are built from filled blocks
CASES = {}
SIZED = []      # the cases with a sibling several times their size (builder(capi, big=True))


def case(name, sized=False):
    def register(f):
        CASES[name] = f
        if sized:
            SIZED.append(name)
        return f
    return register


def _fit_case(kind):
    def build(capi, big=False):
        def cloud(n):
            if kind == 0:
                return synth.plane_cloud_c1(n, 31), None
            if kind == 1:
                return synth.sphere_cloud_c3(n, 32), None
            return synth.cylinder_cloud_c3(n, 33)
        clouds = [cloud(n) for n in ((20011,) if big else (777, 4097))]
        return lambda: [capi.fit(kind, p, q, threshold=0.01, max_iteration=300, probability=prob, seed=7 + len(p))
                        for p, q in clouds for prob in (1.0, 0.99)]
    return build


for _kind, _name in enumerate(("plane", "sphere", "cylinder")):
    case("fit_" + _name, sized=True)(_fit_case(_kind))


@case("segment_plane_iterative", sized=True)
def _(capi, big=False):
    pts = synth.room_cloud_c5(15001 if big else 2049)
    return lambda: capi.segment_plane_iterative(pts, 0.02, max_iteration=100, min_ratio=0.05, seed=3)


@case("match_mutual_nn", sized=True)
def _(capi, big=False):
    from test_gpu_match_sliced import _pair
    fs, fd = _pair(np.random.default_rng(5), *((6001, 4001) if big else (1537, 1025)))

    def run():
        out = []
        for mode in (0, 2):
            old = capi.set_config(match_pipeline=mode)
            try:
                out.append(capi.match_mutual_nn(fs, fd) + (capi.match_last_path(), capi.match_last_fallbacks()))
            finally:
                capi.restore_config(old)
        assert not out[0][2] & 2 and out[1][2] & 2          # bit 1: the matrices went up in slices
        return out
    return run


@case("registration_ransac", sized=True)
def _(capi, big=False):
    from test_gpu_registration import _problem
    d, cs, cd = _problem(n=12001, m=3200) if big else _problem()

    def run():
        out = []
        for cache in (2, 0):
            old = capi.set_config(reg_cache=cache)
            try:
                out.append(capi.registration_ransac(d["src"], d["dst"], cs, cd, threshold=0.03, max_iter=3000,
                                                    edge_length_threshold=0.9, confidence=0.999, seed=17))
            finally:
                capi.restore_config(old)
        used = [st["lds_wave_hypotheses"] + st["global_wave_hypotheses"] for _, st in out]
        assert used[0] > 0 and used[1] == 0          # the candidate cache answered or walked pairs when forced, none when off
        return out
    return run


def _reg_pair(n, seed):
    d = synth.registration_pair_c4(n, seed=seed, dim=33, sigma=0.001)
    inv = np.empty(n, dtype=np.int64)
    inv[d["perm"]] = np.arange(n)
    return d, inv


@case("kabsch")
def _(capi, big=False):
    d, inv = _reg_pair(3000, 13)
    src, dst = d["src"][:1031], np.ascontiguousarray(d["dst"][inv][:1031])
    return lambda: [capi.kabsch(src, dst, scaling) for scaling in (False, True)]


@case("information_matrix")
def _(capi, big=False):
    d, _ = _reg_pair(3000, 13)
    return lambda: [capi.information_matrix(d["src"], d["dst"], 0.03, T) for T in (d["T"], np.eye(4))]


def _icp_inputs(big, colored=False):
    import colored_icp_ref_util as cu
    import icp_ref_util as iu
    u = cu if colored else iu
    return [u.sized_case(6001)] if big else [u.sized_case(257), u.case("nonfinite")]


@case("registration_icp", sized=True)
def _(capi, big=False):
    cs = _icp_inputs(big)
    return lambda: [capi.registration_icp(c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"], want_correspondences=True)
                    for c in cs]


def _icp_plane(l1):
    def build(capi, big=False):
        cs = _icp_inputs(big)
        return lambda: [capi.registration_icp_plane(c["src"], c["dst"], c["dst_normals"], c["max_dist"], c["init"], c["max_iteration"],
                                                    want_correspondences=True, l1=l1) for c in cs]
    return build


case("registration_icp_plane", sized=True)(_icp_plane(False))
case("registration_icp_plane_l1", sized=True)(_icp_plane(True))


@case("registration_icp_colored", sized=True)
def _(capi, big=False):
    import colored_icp_ref_util as cu
    cs = _icp_inputs(big, colored=True)[:1]       # n257 (n6001)
    return lambda: [capi.registration_icp_colored(c["src"], c["src_colors"], c["dst"], c["dst_normals"], c["dst_colors"], c["max_dist"],
                                                  c["init"], cu.LAMBDA, c["max_iteration"], want_correspondences=True) for c in cs]


@case("multi_scale_icp", sized=True)
def _(capi, big=False):
    import icp_ref_util as iu
    m = iu.multi_case(12001 if big else 3000)
    vs, its = iu.levels_of(m["voxel"], True)
    return lambda: capi.multi_scale_icp(m["src"], m["dst"], vs, its, m["max_dist"], m["init"], 1, m["dst_normals"])


@case("global_registration")
def _(capi, big=False):
    d, _ = _reg_pair(2000, 13)
    return lambda: capi.global_registration(d["src"], d["dst"], d["feat_src"], d["feat_dst"], voxel_size=0.03 / 1.4, max_iter=3000,
                                            seed=3, want_stats=True)


@case("normals_from_map")
def _(capi, big=False):
    from test_gpu_normals import _depth_map
    xyz = _depth_map(65, 47, seed=9)
    return lambda: [capi.normals_from_map(xyz, 65, 47, k, (0.1, -0.2, -0.5)) for k in (5, 2)]


@case("detect_boundary_points")
def _(capi, big=False):
    import boundary_ref_util as bu
    pts, nrm = bu.shell(257, seed=17)
    return lambda: [capi.detect_boundary_points(pts, normals, search, radius, max_nn, 90.0)
                    for normals in (nrm, None)
                    for search, radius, max_nn in ((capi.SEARCH_HYBRID, 0.5, 30), (capi.SEARCH_KNN, 0.0, 12), (capi.SEARCH_RADIUS, 0.4, 0))]


def _knn(capi, data, q, searches, paths):
    ix = capi.KnnIndex(data)
    try:
        out = [ix.search(q, k, search, radius, stats=True) for k, search, radius in searches]
    finally:
        ix.close()
    assert [r[-1]["path"] for r in out] == list(paths)
    return out


@case("knn_grid", sized=True)
def _(capi, big=False):
    rng = np.random.default_rng(24)
    data, q = rng.standard_normal((6001 if big else 1200, 3)), rng.standard_normal((1031, 3))
    q[100, 1], q[511, 2], q[512, 0] = np.nan, np.inf, -np.inf
    dist = _knn(capi, data, q, [(17, capi.KNN_SEARCH_KNN, 0.0)], [capi.KNN_PATH_GRID])[0][1]
    radius = float(np.nanmedian(dist[:, 8]))        # about half of the lists are cut
    return lambda: _knn(capi, data, q, [(17, capi.KNN_SEARCH_KNN, 0.0), (17, capi.KNN_SEARCH_HYBRID, radius)], [capi.KNN_PATH_GRID] * 2)


@case("knn_tile", sized=True)
def _(capi, big=False):
    import knn_seam_cases as sc
    data, q = sc.chunk_input(dict(sc.TILE_CHUNKS, n=3001) if big else sc.TILE_CHUNKS, 21)
    return lambda: _knn(capi, data, q, [(3, capi.KNN_SEARCH_KNN, 0.0), (130, capi.KNN_SEARCH_KNN, 0.0)],
                        [capi.KNN_PATH_TILE, capi.KNN_PATH_SELECT])


def _fpfh_clouds():
    import fpfh_ref_util as fu
    p, q = fu.three_surface_cloud(2000)
    tp, tq = fu.three_surface_cloud(65, seed=65)
    return (p, q), (tp, tq)


@case("estimate_normals")
def _(capi, big=False):
    (p, _), (tp, _) = _fpfh_clouds()
    return lambda: [capi.estimate_normals(p, capi.SEARCH_HYBRID, 0.2, 30, stats=True),
                    capi.estimate_normals(p, capi.SEARCH_KNN, 0.0, 17, orient_to=(0.0, 0.0, 0.0), stats=True),
                    capi.estimate_normals(tp, capi.SEARCH_KNN, 0.0, 30, stats=True)]


def _fpfh(search, radius, max_nn):
    def build(capi, big=False):
        (p, q), (tp, tq) = _fpfh_clouds()
        return lambda: [capi.compute_fpfh_feature(p, q, search, radius, max_nn, stats=True),
                        capi.compute_fpfh_feature(tp, tq, search, 10.0 if radius else 0.0, max_nn, stats=True)]
    return build


case("compute_fpfh_hybrid")(_fpfh(2, 0.25, 100))
case("compute_fpfh_knn")(_fpfh(0, 0.0, 33))


@case("preprocess_fragment")
def _(capi, big=False):
    (p, q), _ = _fpfh_clouds()
    return lambda: [capi.preprocess_fragment(p, 0.05, stats=True), capi.preprocess_fragment(p, 0.05, normals=q, stats=True)]


@case("fpfh_stages")
def _(capi, big=False):
    # the stage hook of tests/test_gpu_fpfh_stages.py: non-finite points, whose SPFH rows the device never writes, and lists
    # with unused tails (max_nn above the Hybrid count, and above the 65 points of the small cloud)
    import fpfh_stage_util as su
    (p, q), (tp, tq) = _fpfh_clouds()
    p, q, _ = su.with_nonfinite(p, q)
    tp, tq, _ = su.with_nonfinite(tp, tq)
    return lambda: [capi.fpfh_stages(p, q, capi.SEARCH_HYBRID, 0.25, 100), capi.fpfh_stages(tp, tq, capi.SEARCH_KNN, 0.0, 128)]


def _voxel_inputs():
    import voxel_ref_util as vu
    pts, cell = vu.voxel_seam_cloud(257, 4096, vu.SEAM_HEAD)
    return pts, vu.seam_normals(cell)


def _voxel(path):
    def build(capi, big=False):
        pts, nrm = _voxel_inputs()

        def run():
            capi.voxel_force_path(path)
            try:
                out = capi.voxel_down_sample(pts, 1.0, normals=nrm, trace=True, stats=True)
            finally:
                capi.voxel_force_path(0)
            assert out[1]["path"] == (path or capi.VOXEL_PATH_PACKED)
            return out
        return run
    return build


case("voxel_down_sample")(_voxel(0))
case("voxel_down_sample_wide")(_voxel(2))


@case("voxel_down_sample_multi")
def _(capi, big=False):
    pts, nrm = _voxel_inputs()
    return lambda: capi.voxel_down_sample_multi(pts, [1.0, 2.0], normals=nrm, trace=True, stats=True)


def _fps(n, path):
    def build(capi, big=False):
        import fps_ref_util as fu
        pts = fu.fps_seam_cloud(n)

        def run():
            out = capi.farthest_point_sampling(pts, 64, stats=True)
            assert out[1]["path"] == path
            return out
        return run
    return build


case("farthest_point_sampling_single")(_fps(1025, 1))
case("farthest_point_sampling_tiles")(_fps(8193, 2))


def _quirk_cloud():
    """the quirk cloud of tests/test_gpu_proximity.py: duplicates, NaN and +-inf rows, unnormalised normals"""
    rng = np.random.default_rng(4)
    xyz = rng.uniform(0, 1, (4000, 3))
    xyz[rng.integers(0, 4000, 500)] = xyz[rng.integers(0, 4000, 500)]
    xyz[10, 0] = np.nan
    xyz[20] = np.inf
    xyz[30, 2] = -np.inf
    nrm = rng.standard_normal((4000, 3)) * rng.uniform(0.5, 1.5, (4000, 1))
    nrm[40] = np.nan
    return xyz, nrm


PROX_EVALUATORS = (dict(kind="distance", dist=0.04), dict(kind="distance_normals", dist=0.05, angle_deg=60.0),
                   dict(kind="normals", angle_deg=-70.0))


@case("proximity_segment")
def _(capi, big=False):
    xyz, nrm = _quirk_cloud()
    return lambda: [capi.proximity_segment(xyz, 0.05, normals=None if kw["kind"] == "distance" else nrm, stats=True, **kw)
                    for kw in PROX_EVALUATORS]


@case("proximity_segment_nn")
def _(capi, big=False):
    xyz, nrm = _quirk_cloud()
    xyz, nrm = xyz[50:2050], nrm[50:2050]                       # (finite rows: the lists come from radius_neighbors)
    off, idx, _ = capi.radius_neighbors(xyz, 0.05)
    return lambda: [capi.proximity_segment_nn(xyz, off, idx, normals=None if kw["kind"] == "distance" else nrm, stats=True, **kw)
                    for kw in PROX_EVALUATORS]


@case("radius_neighbors")
def _(capi, big=False):
    xyz = _quirk_cloud()[0][:2000]
    return lambda: capi.radius_neighbors(xyz, 0.05)


@case("raycast_pinhole")
def _(capi, big=False):
    import raycast_ref_util as ru
    scenes = ru.scenes()
    picked = [scenes[k] for k in ("257 triangles", "empty mesh between", "65 x 9")]
    meshes, frames = ru.BATCH_MESHES(), ru.BATCH_FRAMES()
    return lambda: ([capi.raycast_pinhole(m, [poses], cam, stats=True) for m, poses, cam, _ in picked] +
                    [capi.raycast_pinhole(meshes, frames, ru.CAM, stats=True)])


@case("ppf_model_table")
def _(capi, big=False):
    import ppf_ref_util as pu
    n = min(s for s in pu.TABLE_SIZES if s > 64)
    pts, nrm, diameter, r_min = pu.model_case("random", n, 100 + n)

    def run():
        m = capi.PpfModel(pts, nrm, diameter, r_min)
        try:
            return m.table()
        finally:
            m.close()
    return run


def _vote(capi, pu, c, device_memory, max_groups):
    capi.ppf_force(device_memory, max_groups)
    try:
        m = pu.lib_model(capi, c)
        try:
            out = pu.lib_vote(m, c, stats=True)
        finally:
            m.close()
    finally:
        capi.ppf_force(False, 0)
    assert not device_memory or out[1]["path"] == capi.PPF_PATH_DEVICE
    assert not max_groups or out[1]["groups"] <= max_groups
    return out


@case("ppf_vote", sized=True)
def _(capi, big=False):
    import ppf_ref_util as pu
    if big:
        pts, nrm, diameter, r_min, sp, sn, ref, _ = pu.vote_case("box", n=3600, n_ref=12, clutter=1200)
        cs = [pu._case((pts, nrm, diameter, r_min), pu.params(angle_step=pu.ANGLE_STEPS["6"]), (sp, sn), ref)]
    else:
        cs = [pu.case("count_random_65"), pu.case("lds_edge_plus_1")]
    return lambda: [_vote(capi, pu, c, dm, mg) for c in cs for dm, mg in ((False, 0), (True, 0), (False, 3), (True, 3))]


@case("ppf_vote_edges")
def _(capi, big=False):
    import ppf_edge_ref_util as eu
    import ppf_ref_util as pu
    c = eu.case("count_random_65")

    def run():
        m = pu.lib_model(capi, c)
        try:
            return [m.table(), pu.lib_vote(m, c, stats=True)] + [_vote(capi, pu, c, True, 3)]
        finally:
            m.close()
    return run


@case("ppf_cluster_poses", sized=True)
def _(capi, big=False):
    import ppf_cluster_ref_util as cu
    names = ("blobs_2049",) if big else ("blobs_257", "chain")

    def run():
        out = []
        for name in names:
            for splits in (1, 3):
                capi.ppf_cluster_force(splits)
                try:
                    out.append(capi.ppf_cluster_poses(*cu.family(name), dist_threshold=cu.R_DIST, angle_threshold=cu.ANGLE))
                finally:
                    capi.ppf_cluster_force(0)
        return out
    return run


@case("ppf_estimate")
def _(capi, big=False):
    import ppf_cluster_ref_util as cu
    c = cu.estimate_case()

    def run():
        m = capi.PpfModel(c["points"], c["normals"], c["diameter"], c["r_min"])
        try:
            return capi.ppf_estimate(m, c["scene_points"], c["scene_normals"], c["reference"], score_thresh=0.0,
                                     refine_method="PointToPlane", angle_threshold=cu.ANGLE)
        finally:
            m.close()
    return run


@case("ppf_prepare_scene")
def _(capi, big=False):
    import ppf_edge_ref_util as eu
    pts, nrm, _, _, _ = eu.plate_with_holes(n_side=84, seed=11)      # the cloud of tests/test_gpu_ppf_prepare.py
    rng = np.random.default_rng(12)
    pts = pts + np.array([0.1, -0.2, 1.5]) + rng.normal(0, 0.002, size=pts.shape)
    nrm = nrm * rng.choice([-1.0, 1.0], size=(len(nrm), 1)) * rng.uniform(0.5, 2.0, size=(len(nrm), 1))
    bad = rng.choice(len(pts), size=37, replace=False)
    pts[bad[:20], rng.integers(0, 3, size=20)] = np.nan
    pts[bad[20:30], rng.integers(0, 3, size=10)] = np.inf
    pts[bad[30:], rng.integers(0, 3, size=7)] = -np.inf
    pts, nrm = np.ascontiguousarray(pts), np.ascontiguousarray(nrm)
    return lambda: [capi.ppf_prepare_scene(pts, normals, 1.22, 0.05, 0.05, 0.02, 30) for normals in (nrm, None)]


# ---- running the panel ------------------------------------------------------------------------------------------------------
_RUNS, _BASELINES = {}, {}


def _run_of(capi, name, big=False):
    if (name, big) not in _RUNS:
        assert capi._scratch_pattern == -1          # inputs (and what a builder computes on the device) are made with the hook off
        _RUNS[(name, big)] = CASES[name](capi, big) if big else CASES[name](capi)
    return _RUNS[(name, big)]


def _baseline(capi, name):
    """the case with the hook off, twice: a baseline that differs from itself is a finding of its own"""
    if name not in _BASELINES:
        run = _run_of(capi, name)
        first, second = _freeze(run()), _freeze(run())
        assert not _differences(first, second), (name, "two unfilled runs differ", _differences(first, second))
        _BASELINES[name] = first
    return _BASELINES[name]


def _filled(capi, run, pattern):
    """-> (frozen result, blocks filled) of one run under the fill"""
    with capi.scratch_fill(pattern):
        got = _freeze(run())
        blocks, nbytes = capi.scratch_fill_stats()
    return got, blocks


def test_fill_reaches_fresh_and_recycled_blocks(capi):
    """a dead hook would make everything below pass"""
    capi.lib().m3d_release_cached(0)          # nothing parked: the first probe is a fresh allocation, the second takes its block
    with capi.scratch_fill(0xA5):
        assert capi.scratch_probe(PROBE_BYTES).tolist() == [0xA5] * 128
        blocks, nbytes = capi.scratch_fill_stats()
        assert blocks == 1 and nbytes >= PROBE_BYTES
        with capi.scratch_fill(0x5A):
            assert capi.scratch_fill_stats() == (0, 0)
            assert capi.scratch_probe(PROBE_BYTES).tolist() == [0x5A] * 128
            assert capi.scratch_fill_stats() == (1, nbytes)          # the same block, from the free list
        with capi.scratch_fill(-1):
            assert capi.scratch_probe(PROBE_BYTES).tolist() == [0x5A] * 128     # handed out as it was left
            assert capi.scratch_fill_stats() == (0, 0)
    assert capi.scratch_fill_stats() == (0, 0)
    for bad in (-2, 256):
        assert capi.lib().m3d_bench_scratch_fill(bad) == capi.ERR_INVALID_ARG
    with pytest.raises(ZeroDivisionError):
        with capi.scratch_fill(0x11):
            1 / 0
    assert capi._scratch_pattern == -1
    capi.scratch_probe(PROBE_BYTES)
    assert capi.scratch_fill_stats() == (0, 0)      # restored on an exception as well


@pytest.mark.parametrize("name,pattern", [(n, p) for p in PATTERNS for n in CASES], ids=lambda v: v if isinstance(v, str) else "0x%02X" % v)
def test_panel(capi, name, pattern):
    want = _baseline(capi, name)
    got, blocks = _filled(capi, _run_of(capi, name), pattern)
    assert blocks > 0, (name, "takes no block from the pool")
    assert not _differences(got, want), (name, "0x%02X" % pattern, _differences(got, want))


@pytest.mark.parametrize("pattern", (-1, 0xFF), ids=("off", "0xFF"))
@pytest.mark.parametrize("name", SIZED)
def test_small_after_large(capi, name, pattern):
    """scratch that lives in the lane context and grows only: laid out for the large call, read by the small one"""
    small, large = _run_of(capi, name), _run_of(capi, name, big=True)
    with capi.scratch_fill(pattern):
        first = _freeze(small())
        large()
        again = _freeze(small())
    assert not _differences(first, again), (name, _differences(first, again))
    assert not _differences(first, _baseline(capi, name)), (name, _differences(first, _baseline(capi, name)))


def test_two_threads_under_a_fill(capi):
    """lanes interleave: a fill on one lane waits for the device while the other lane's kernels run"""
    names = ("compute_fpfh_hybrid", "proximity_segment")
    want = {n: _baseline(capi, n) for n in names}
    runs = {n: _run_of(capi, n) for n in names}
    got, errors = {n: [] for n in names}, []

    def work(n):
        try:
            for _ in range(3):
                got[n].append(_freeze(runs[n]()))
        except Exception as e:   # noqa: BLE001
            errors.append((n, repr(e)))

    with capi.scratch_fill(0x3F):
        threads = [threading.Thread(target=work, args=(n,)) for n in names]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        blocks, _ = capi.scratch_fill_stats()
    assert not errors, errors
    assert blocks > 0
    for n in names:
        assert len(got[n]) == 3
        for k, g in enumerate(got[n]):
            assert not _differences(g, want[n]), (n, k, _differences(g, want[n]))
