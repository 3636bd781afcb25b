"""misc3d_amd -- MI355X (gfx950) implementation of the Misc3D RANSAC hot path.

Drop-in for the reference's python API on this path (module layout of python/py_misc3d.cpp:25-62):

    import misc3d_amd as m3d
    w, index = m3d.common.fit_plane(pcd, 0.01, 100)
    w, index = m3d.common.fit_sphere(pcd, 0.01, 100)
    w, index = m3d.common.fit_cylinder(pcd, 0.01, 100)
    results  = m3d.segmentation.segment_plane_iterative(pcd, 0.01, 100, 0.1)
    idx      = m3d.registration.match_correspondence(fpfh_src, fpfh_dst)
    T        = m3d.registration.compute_transformation_ransac(src, dst, idx, 0.03, 100000)
    T        = m3d.registration.compute_transformation_least_square(src, dst)
    T, info  = m3d.registration_icp(src, dst, 0.02, T)      # the Open3D call the reference's examples chain next
    index    = m3d.features.detect_boundary_points(plane, ("hybrid", 0.02, 30))
    normals  = m3d.features.estimate_normals(pcd, ("hybrid", 0.1, 30), orient_to=(0, 0, 0))   # unorganised clouds
    fpfh     = m3d.features.compute_fpfh_feature(pcd, ("hybrid", 0.25, 100))                  # (33, N), Open3D's Feature.data
    normals, fpfh = m3d.reconstruction.preprocess_fragment(fragment, voxel_size)              # pipeline.cpp:379-401
    points, normals, colors = m3d.preprocessing.voxel_down_sample(pcd, 0.005)   # Open3D's first call of every example
    index    = m3d.preprocessing.farthest_point_sampling(pcd, 1000)
    roi      = m3d.preprocessing.crop_roi_pointcloud(pcd, (tl_x, tl_y, br_x, br_y), (width, height))
    normals  = m3d.common.estimate_normals(pcd, (848, 480), 3)
    ok, T, info = m3d.reconstruction.global_registration(frag_s, frag_t, fpfh_s, fpfh_t, voxel_size)   # pipeline.cpp:790-828
    results  = m3d.reconstruction.register_fragment_pairs(fragments, fpfhs, voxel_size=voxel_size)     # pipeline.cpp:428-439
    T, info  = m3d.reconstruction.fragment_odometry(frag_s, frag_t, voxel_size, init)                  # pipeline.cpp:754-763
    T, info  = m3d.reconstruction.refine_fragment_pair(frag_s, frag_t, voxel_size, edge_pose)          # pipeline.cpp:686-697
    renderer = m3d.pose_estimation.RayCastRenderer(intrinsic); renderer.cast_rays([mesh, mesh], [pose, pose2])
    depth    = renderer.get_depth_map().numpy(); instance = renderer.get_instance_map().numpy()        # ray_cast_renderer.cpp
    voting   = m3d.pose_estimation.PPFVoting(model_points, model_normals, diameter, r_min)             # ppf_estimation.cpp:603-640
    poses, num_votes, corr_mi, reference = voting.vote(scene_points, scene_normals, reference_indices) # ppf_estimation.cpp:399-524
    ppf      = m3d.pose_estimation.PPFEstimator(m3d.pose_estimation.PPFEstimatorConfig()); ppf.train(model_points)   # ppf_estimation.cpp:526-601
    ret, results = ppf.estimate(scene_points); pose = results[0].pose                                 # ppf_estimation.cpp:280-397

Layout (only what the path needs):
  csrc/      HIP kernels, host driver, C ABI            -> lib/libmisc3d_amd.so
  host/      pybind11 module over include/misc3d/**      -> _py_misc3d*.so  (this API)
  capi.py    ctypes binding of include/misc3d_amd.h      (tests, bench, distributed driver)
  distributed.py  hypothesis sharding over torch.distributed (RCCL)
  synth.py   seeded synthetic clouds of the BASELINE.json configurations

There is no CPU fallback: the native libraries must be built (python __graft_entry__.py) and every
compute call needs a HIP device.
"""
__version__ = "0.1.0"

import enum as _enum

try:
    from . import _py_misc3d as _ext
except ImportError as e:  # fail loudly: no pure-python stand-in exists
    raise ImportError(
        "misc3d_amd: the native host module misc3d_amd/_py_misc3d*.so (or lib/libmisc3d_amd.so) is missing or "
        f"failed to load ({e}). Build with `python __graft_entry__.py`.") from e

common = _ext.common
registration = _ext.registration
segmentation = _ext.segmentation
VerbosityLevel = _ext.VerbosityLevel
set_verbosity_level = _ext.set_verbosity_level
release_host_scratch = _ext.release_host_scratch   # frees the page-locked blocks kept between calls ("Page-locked memory")
get_verbosity_level = _ext.get_verbosity_level
device_count = _ext.device_count
Error, Warning, Info, Debug = (VerbosityLevel.Error, VerbosityLevel.Warning, VerbosityLevel.Info,
                               VerbosityLevel.Debug)



def registration_icp(source, target, max_correspondence_distance, init=None, max_iteration=30,
                     relative_fitness=1e-6, relative_rmse=1e-6, device=0, estimation="point_to_point"):
    """ICP = open3d.pipelines.registration.registration_icp(source, target, max_correspondence_distance, init,
    estimation, ICPConvergenceCriteria(...)).  estimation="point_to_point" (the default):
    TransformationEstimationPointToPoint(), which the reference's examples run on the pose of compute_transformation_ransac
    (examples/cpp/transform_estimation.cpp:82-86); source / target: (N, 3) arrays or objects with `.points`.
    estimation="point_to_plane": TransformationEstimationPointToPlane(), MultiScaleICP's Point2PlaneICP
    (src/pipeline.cpp:949-955); the target then carries normals: a (points, normals) tuple or an object with .points /
    .normals (RuntimeError without them).
    estimation="point_to_plane_l1": TransformationEstimationPointToPlane(L1Loss()), the PointToPlane refinement of
    PPFEstimator (src/ppf_estimation.cpp:937-990); the target carries normals in the same way.
    Returns (4x4 pose, dict(fitness, inlier_rmse, correspondences, iterations, converged))."""
    import numpy as _np

    from . import capi as _capi
    if estimation == "point_to_point":
        pts = [_np.asarray(getattr(c, "points", c), dtype=_np.float64).reshape(-1, 3) for c in (source, target)]
        return _capi.registration_icp(pts[0], pts[1], max_correspondence_distance, init, max_iteration,
                                      relative_fitness, relative_rmse, device)
    if estimation not in ("point_to_plane", "point_to_plane_l1"):
        raise RuntimeError('[Misc3D Error] estimation: "point_to_point", "point_to_plane" or "point_to_plane_l1"')
    src, _ = _points_normals(source)
    dst, nrm = _points_normals(target)
    try:
        return _capi.registration_icp_plane(src, dst, nrm, max_correspondence_distance, init, max_iteration,
                                            relative_fitness, relative_rmse, device, l1=estimation == "point_to_plane_l1")
    except _capi.M3DError as e:
        raise RuntimeError(str(e)) from e


def registration_colored_icp(source, target, max_correspondence_distance, init=None, lambda_geometric=0.968, max_iteration=30,
                             relative_fitness=1e-6, relative_rmse=1e-6, device=0):
    """open3d.pipelines.registration.registration_colored_icp(source, target, max_correspondence_distance, init,
    TransformationEstimationForColoredICP(lambda_geometric), ICPConvergenceCriteria(...)): MultiScaleICP's ColoredICP, the
    reference's default (src/pipeline.cpp:956-962).  source / target: (points, normals, colors) tuples or objects with
    .points / .normals / .colors; the source needs colours, the target normals and colours (RuntimeError without them).
    Returns (4x4 pose, dict(fitness, inlier_rmse, correspondences, iterations, converged)), as registration_icp does."""
    from . import capi as _capi
    src, _, sc = _points_normals_colors(source)
    dst, nrm, dc = _points_normals_colors(target)
    try:
        return _capi.registration_icp_colored(src, sc, dst, nrm, dc, max_correspondence_distance, init, lambda_geometric,
                                              max_iteration, relative_fitness, relative_rmse, device)
    except _capi.M3DError as e:
        raise RuntimeError(str(e)) from e


def _search_param(param):
    """An open3d KDTreeSearchParamHybrid / KDTreeSearchParamRadius / KDTreeSearchParamKNN (anything with .radius and
    optionally .max_nn, or with .knn), or a tuple ("hybrid", radius, max_nn) / ("radius", radius) / ("knn", k)
    -> (kind, radius, max_nn)."""
    if isinstance(param, tuple):
        kind = str(param[0]).lower()
        if kind == "knn":
            radius, max_nn = 0.0, int(param[1])
        else:
            radius = float(param[1])
            max_nn = int(param[2]) if len(param) > 2 else 0
    elif hasattr(param, "knn") and not hasattr(param, "radius"):
        kind, radius, max_nn = "knn", 0.0, int(param.knn)
    else:
        radius = float(param.radius)
        max_nn = int(getattr(param, "max_nn", 0))
        kind = "hybrid" if hasattr(param, "max_nn") else "radius"
    if kind not in ("hybrid", "radius", "knn"):
        raise RuntimeError("[Misc3D Error] param: KDTreeSearchParamHybrid / KDTreeSearchParamRadius / KDTreeSearchParamKNN")
    return kind, radius, max_nn


def _points_normals(pc):
    """(N, 3) array, (points, normals) tuple or an object with .points / .normals -> (points, normals or None)"""
    import numpy as _np
    if isinstance(pc, tuple) and len(pc) == 2:
        pts, nrm = pc
    else:
        pts, nrm = getattr(pc, "points", pc), getattr(pc, "normals", None)
    pts = _np.asarray(pts, dtype=_np.float64).reshape(-1, 3)
    if nrm is not None:
        nrm = _np.asarray(nrm, dtype=_np.float64).reshape(-1, 3)
        if len(nrm) != len(pts) or len(nrm) == 0:
            nrm = None
    return pts, nrm


def _points_normals_colors(pc):
    """_points_normals, and a (points, normals, colors) tuple or an object's .colors -> (points, normals, colors); an entry
    that is missing, empty or of another length is None"""
    import numpy as _np
    if isinstance(pc, tuple) and len(pc) == 3 and _np.ndim(pc[0]) == 2:   # (three bare points stay an array of points)
        pts, nrm = _points_normals((pc[0], pc[1]))
        col = pc[2]
    else:
        pts, nrm = _points_normals(pc)
        col = None if isinstance(pc, tuple) else getattr(pc, "colors", None)
    if col is not None:
        col = _np.asarray(col, dtype=_np.float64).reshape(-1, 3)
        if len(col) != len(pts) or len(col) == 0:
            col = None
    return pts, nrm, col


class _Features:
    """misc3d.features (python/py_features.cpp): detect_boundary_points; and the two Open3D calls every registration entry
    point depends on: estimate_normals (unorganised clouds) and compute_fpfh_feature"""

    @staticmethod
    def detect_boundary_points(pc, param=("hybrid", 0.01, 30), angle_threshold=90.0, device=0):
        """DetectBoundaryPoints (src/boundary_detection.cpp:68-113).  pc: (N, 3) array, (points, normals) tuple or
        an object with .points / .normals.  param: an open3d KDTreeSearchParamHybrid / KDTreeSearchParamRadius /
        KDTreeSearchParamKNN (anything with .radius and optionally .max_nn, or with .knn), or a tuple
        ("hybrid", radius, max_nn) / ("radius", radius) / ("knn", k).
        Returns the list of boundary point indices (ascending)."""
        import numpy as _np

        from . import capi as _capi
        pts, nrm = _points_normals(pc)
        kind, radius, max_nn = _search_param(param)
        search = {"hybrid": _capi.SEARCH_HYBRID, "radius": _capi.SEARCH_RADIUS, "knn": _capi.SEARCH_KNN}[kind]
        try:
            idx = _capi.detect_boundary_points(pts, nrm, search, radius, max_nn, angle_threshold, device)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e
        return [int(i) for i in idx]

    @staticmethod
    def estimate_normals(pc, param=("hybrid", 0.1, 30), *, orient_to=None, device=0):
        """open3d PointCloud.estimate_normals(param) for an unorganised cloud (+ orient_normals_towards_camera_location(
        orient_to) when given).  pc: (N, 3) array or an object with .points; param as detect_boundary_points takes it
        (Hybrid or KNN).  Returns the (N, 3) normals."""
        from . import capi as _capi
        kind, radius, max_nn = _search_param(param)
        try:
            return _capi.estimate_normals(_xyz(pc), _SEARCH[kind], radius, max_nn, orient_to, device)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e

    @staticmethod
    def compute_fpfh_feature(pc, param=("hybrid", 0.25, 100), *, device=0):
        """open3d.pipelines.registration.compute_fpfh_feature(pc, param).  pc: a (points, normals) tuple or an object with
        .points / .normals.  Returns a (33, N) array laid out as Open3D's Feature.data (Fortran order: the transposed view of
        the (N, 33) rows), accepted as is by registration.match_correspondence and reconstruction.global_registration."""
        from . import capi as _capi
        pts, nrm = _points_normals(pc)
        kind, radius, max_nn = _search_param(param)
        try:
            return _capi.compute_fpfh_feature(pts, nrm, _SEARCH[kind], radius, max_nn, device).T
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e


_SEARCH = {"knn": 0, "radius": 1, "hybrid": 2}   # capi.SEARCH_*
features = _Features()


def _xyz(c):
    import numpy as _np
    return _np.ascontiguousarray(_np.asarray(getattr(c, "points", c), dtype=_np.float64).reshape(-1, 3))


def _feat(f, n):
    """open3d Feature (.data: dim x N) or an ndarray, (N, dim) or (dim, N) -> (N, dim) C-contiguous"""
    import numpy as _np
    is_feature = not isinstance(f, _np.ndarray) and hasattr(f, "data")      # (an ndarray has a .data of its own: its buffer)
    a = _np.asarray(f.data if is_feature else f, dtype=_np.float64)
    if is_feature or (a.ndim == 2 and a.shape[0] != n and a.shape[1] == n):
        a = a.T          # Eigen dim x N column-major == (N, dim) row-major: a transposed VIEW of the same memory
    return _np.ascontiguousarray(a)


class LocalRefineMethod(_enum.IntEnum):
    """PipelineConfig::LocalRefineMethod (include/misc3d/reconstruction/pipeline_config.h:23-28)"""
    Point2PointICP = 0
    Point2PlaneICP = 1
    ColoredICP = 2        # the reference's default; accelerated when both clouds carry colours (m3d_multi_scale_icp_colored)
    GeneralizedICP = 3    # not accelerated


_REFINE_METHODS = {"point_to_point": 0, "point_to_plane": 1, "colored": 2, "generalized": 3}


def _refine_method(method):
    if isinstance(method, str):
        if method not in _REFINE_METHODS:
            raise RuntimeError("[Misc3D Error] Unknown local refine method.")
        return _REFINE_METHODS[method]
    return int(method)


class _Reconstruction:
    """misc3d.reconstruction, the registration half of ReconstructionPipeline (src/pipeline.cpp): PreProcessFragments
    (:379-401), GlobalRegistration (:790-828), the loop over fragment pairs that calls it (:428-439), and MultiScaleICP (:927-982)
    with its two callers, fragment odometry (:754-763) and refinement (:686-697).  Calls release the GIL: Python threads that call
    global_registration / fit_* / match_correspondence side by side run side by side on the device (lanes)."""

    LocalRefineMethod = LocalRefineMethod

    @staticmethod
    def multi_scale_icp(source, target, voxel_sizes, max_iters, max_correspondence_distance, init=None,
                        method="point_to_plane", *, device=0, stats=False, lambda_geometric=0.968):
        """ReconstructionPipeline::MultiScaleICP: per level both clouds voxel-down-sampled from the originals, ICP with
        ICPConvergenceCriteria(1e-6, 1e-6, max_iters[l]) seeded with the previous level's pose; then the information matrix
        of the original clouds at 1.4 voxel_sizes[-1].  source / target: (N, 3) arrays, (points, normals) tuples or objects
        with .points / .normals; method: "point_to_point", "point_to_plane", "colored" or a LocalRefineMethod.  ColoredICP
        runs when both clouds carry colours ((points, normals, colors) tuples or objects with .colors), with
        lambda_geometric; without colours it is refused as before, as GeneralizedICP always is ("not accelerated":
        RuntimeError).  Returns (4x4 pose, 6x6 information), and the per-level stats when stats=True."""
        from . import capi as _capi
        src, sn, sc = _points_normals_colors(source)
        dst, dn, dc = _points_normals_colors(target)
        m = _refine_method(method)
        try:
            if m == _capi.REFINE_COLORED_ICP and sc is not None and dc is not None:
                T, info, levels = _capi.multi_scale_icp_colored(src, sc, dst, dn, dc, voxel_sizes, max_iters,
                                                                max_correspondence_distance, init, lambda_geometric, sn, device)
            else:
                T, info, levels = _capi.multi_scale_icp(src, dst, voxel_sizes, max_iters, max_correspondence_distance, init,
                                                        m, dn, sn, device)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e
        return (T, info, levels) if stats else (T, info)

    @staticmethod
    def refine_fragment_pair(source, target, voxel_size, init=None, method="point_to_plane", *, device=0, stats=False,
                             lambda_geometric=0.968):
        """RefineFragmentPair's registration (src/pipeline.cpp:686-697): multi_scale_icp with {v, v/2, v/4} -- formed in
        single precision, as the reference's `const float voxel_size` forms them -- max iterations {50, 30, 15} and
        max_correspondence_distance = 1.4 voxel_size (the single-precision value, as config_.voxel_size_ is); init: the pose-graph edge's pose."""
        import numpy as _np
        v = _np.float32(voxel_size)
        sizes = [float(v), float(v / _np.float32(2.0)), float(v / _np.float32(4.0))]
        return _Reconstruction.multi_scale_icp(source, target, sizes, [50, 30, 15], float(v) * 1.4, init, method,
                                               device=device, stats=stats, lambda_geometric=lambda_geometric)

    @staticmethod
    def fragment_odometry(source, target, voxel_size, init=None, method="point_to_plane", *, device=0, stats=False,
                          lambda_geometric=0.968):
        """RegisterFragmentPair for ADJACENT fragments (src/pipeline.cpp:754-763): multi_scale_icp with {v} (in single
        precision), {50} and max_correspondence_distance = 1.4 voxel_size; init: the pose from the fragment pose graph."""
        import numpy as _np
        v = float(_np.float32(voxel_size))
        return _Reconstruction.multi_scale_icp(source, target, [v], [50], v * 1.4, init, method, device=device, stats=stats,
                                               lambda_geometric=lambda_geometric)

    @staticmethod
    def global_registration(source, target, feature_source, feature_target, voxel_size, max_iter=100000,
                            edge_length_threshold=0.9, confidence=0.999, *, seed=None, device=0):
        """ReconstructionPipeline::GlobalRegistration with the Ransac method: match_correspondence ->
        compute_transformation_ransac(1.4 voxel_size) -> information matrix -> accepted unless info[5, 5] / min(Ns, Nt) < 0.3.
        Returns (success, 4x4 pose, 6x6 information)."""
        from . import capi as _capi
        src, dst = _xyz(source), _xyz(target)
        try:
            return _capi.global_registration(src, dst, _feat(feature_source, len(src)), _feat(feature_target, len(dst)),
                                             voxel_size, max_iter, edge_length_threshold, confidence, seed, device)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e

    @staticmethod
    def preprocess_fragment(pc, voxel_size, *, device=0):
        """ReconstructionPipeline::PreProcessFragments for one fragment: normals by Hybrid(2 voxel_size, 30) when pc has
        none, oriented towards the origin, FPFH by Hybrid(5 voxel_size, 100) -- one upload, both searches on the device.
        Returns (normals (N, 3), fpfh (33, N) as features.compute_fpfh_feature returns it)."""
        from . import capi as _capi
        pts, nrm = _points_normals(pc)
        try:
            normals, feat = _capi.preprocess_fragment(pts, voxel_size, nrm, device)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e
        return normals, feat.T

    @staticmethod
    def register_fragment_pairs(fragments, features=None, pairs=None, voxel_size=0.01, max_iter=100000,
                                edge_length_threshold=0.9, confidence=0.999, *, seeds=None, devices=(0,), inflight=0):
        """BuildPoseGraphForScene's loop closures: every (s, t) of `pairs` through global_registration, dealt to `devices`,
        `inflight` pairs at a time per device.  Default pairs: all s < t with t > s + 1 -- the reference sends ADJACENT fragments
        (t == s + 1) to the multi-scale ICP odometry seeded from the fragment pose graph, never to GlobalRegistration
        (src/pipeline.cpp:752-764): that is fragment_odometry; pass `pairs` explicitly to register those here as well.
        features=None: the descriptors are computed first, fragment by fragment, with preprocess_fragment(voxel_size).
        Returns [(s, t, success, pose, information), ...]."""
        from . import capi as _capi
        pts = [_xyz(f) for f in fragments]
        if features is None:
            features = [_Reconstruction.preprocess_fragment(f, voxel_size, device=devices[0])[1] for f in fragments]
        fts = [_feat(f, len(p)) for f, p in zip(features, pts)]
        if pairs is None:
            pairs = [(s, t) for s in range(len(pts)) for t in range(s + 2, len(pts))]
        try:   # (every fragment is uploaded once per device and stays resident for the call)
            res = _capi.register_fragment_pairs(pts, fts, pairs, voxel_size, max_iter, edge_length_threshold, confidence,
                                                seeds, devices, inflight)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e
        return [(s, t) + r for (s, t), r in zip(pairs, res)]


reconstruction = _Reconstruction()


class _Preprocessing:
    """misc3d.preprocessing (python/py_preprocessing.cpp): farthest_point_sampling, crop_roi_pointcloud, project_into_plane;
    and Open3D's voxel_down_sample, the call every example of the reference starts with (+ its multi-level form)"""

    _FPS_INFO = ("This method has been added to Open3D official branch and hence it will be deprecated in the future.")

    @staticmethod
    def farthest_point_sampling(pc, num_points, *, as_arrays=False, device=0):
        """FarthestPointSampling (src/filter.cpp:13-52), bit for bit.  pc: (N, 3) array or an object with .points.
        Returns list[int], or an int64 array with as_arrays=True."""
        import numpy as _np

        from . import capi as _capi
        _ext._log_info(_Preprocessing._FPS_INFO)   # src/filter.cpp:15-17
        try:
            idx = _capi.farthest_point_sampling(_xyz(pc), int(num_points), device)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e
        if as_arrays:
            return idx.astype(_np.int64)
        return [int(i) for i in idx]

    @staticmethod
    def crop_roi_pointcloud(pc, roi, shape):
        """CropROIPointCloud (src/filter.cpp:54-101): roi = (tl_x, tl_y, br_x, br_y), shape = (width, height) of the
        organised cloud.  Returns an open3d PointCloud (points, and normals / colours when pc has them) when open3d
        imports, else the (K, 3) points array (the fallback of segmentation.segment_plane_iterative)."""
        import numpy as _np

        from . import capi as _capi
        pts = _xyz(pc)
        try:
            idx = _capi.crop_roi_indices(len(pts), roi, shape).astype(_np.int64)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e
        out_pts = pts[idx]
        try:
            import open3d as _o3d
        except ImportError:
            return out_pts
        pcd = _o3d.geometry.PointCloud(_o3d.utility.Vector3dVector(out_pts))
        for attr in ("normals", "colors"):
            v = getattr(pc, attr, None)
            if v is not None:
                v = _np.asarray(v, dtype=_np.float64).reshape(-1, 3)
                if len(v) == len(pts):
                    setattr(pcd, attr, _o3d.utility.Vector3dVector(v[idx]))
        return pcd

    @staticmethod
    def _cloud_arrays(points, normals, colors):
        """points: (N, 3) array or an object with .points (then its .normals / .colors are taken unless given)"""
        import numpy as _np
        if normals is None:
            normals = getattr(points, "normals", None)
        if colors is None:
            colors = getattr(points, "colors", None)
        pts = _xyz(points)
        attrs = []
        for a in (normals, colors):
            if a is not None:
                a = _np.asarray(a, dtype=_np.float64).reshape(-1, 3)
                if len(a) != len(pts) or len(a) == 0:   # (Open3D's HasNormals / HasColors)
                    a = None
            attrs.append(a)
        return pts, attrs[0], attrs[1]

    @staticmethod
    def _voxel_tuple(level, trace):
        import numpy as _np
        out = (level["points"], level["normals"], level["colors"])
        if trace:
            out += (level["first_index"].astype(_np.int64), level["point_to_voxel"].astype(_np.int64))
        return out

    @staticmethod
    def voxel_down_sample(points, voxel_size, normals=None, colors=None, *, trace=False, device=0):
        """open3d PointCloud.voxel_down_sample(voxel_size) on the device, bit for bit the per-voxel means of the reference
        (members added in ascending index).  The voxels come in ascending order of their lowest member index (the
        reference's order is that of an unordered_map).  points: (N, 3) array or an object with .points / .normals /
        .colors.  Returns (points, normals, colors), each (M, 3) or None; with trace=True also first_index (M,) -- the
        lowest member of every voxel -- and point_to_voxel (N,) -- the output row of every input point (what
        voxel_down_sample_and_trace tells), both int64."""
        from . import capi as _capi
        pts, nrm, col = _Preprocessing._cloud_arrays(points, normals, colors)
        try:
            level = _capi.voxel_down_sample(pts, float(voxel_size), nrm, col, device, trace)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e
        return _Preprocessing._voxel_tuple(level, trace)

    @staticmethod
    def voxel_down_sample_multi(points, voxel_sizes, normals=None, colors=None, *, trace=False, device=0):
        """voxel_down_sample at several sizes, every level FROM THE ORIGINAL CLOUD (MultiScaleICP's {v, v/2, v/4},
        src/pipeline.cpp:937-938) with one upload: a list of voxel_down_sample's tuples, each bit for bit the single call's."""
        from . import capi as _capi
        pts, nrm, col = _Preprocessing._cloud_arrays(points, normals, colors)
        try:
            levels = _capi.voxel_down_sample_multi(pts, [float(v) for v in voxel_sizes], nrm, col, device, trace)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e
        return [_Preprocessing._voxel_tuple(level, trace) for level in levels]

    @staticmethod
    def project_into_plane(pc):
        """ProjectIntoPlane: not on the accelerated path (its sums go through Eigen's dynamic-size GEMM, so no exact
        association can be stated for it)."""
        raise RuntimeError(
            "[Misc3D Error] project_into_plane is outside the MI355X-accelerated hot path of this build (its sums go "
            "through Eigen's dynamic-size GEMM: no bit-exact restatement exists); project with numpy instead")


preprocessing = _Preprocessing()


_MAP_ARRAY = None


def _map_array(a):
    """`a` as an ndarray subclass whose .numpy() returns the array itself, so that the reference's
    `renderer.get_depth_map().numpy()` (an open3d.core.Tensor there) runs unchanged"""
    global _MAP_ARRAY
    if _MAP_ARRAY is None:
        import numpy as _np

        class MapArray(_np.ndarray):
            def numpy(self):
                return self
        _MAP_ARRAY = MapArray
    return a.view(_MAP_ARRAY)


def _log_warning(msg):
    if int(get_verbosity_level()) >= int(VerbosityLevel.Warning):
        print(f"[Misc3D WARNING] {msg}")


class RayCastRenderer:
    """misc3d.pose_estimation.RayCastRenderer (src/ray_cast_renderer.cpp; python/py_pose_estimation.cpp:111-118) on the
    device: depth, instance and primitive maps of posed triangle meshes seen by a pinhole camera at the origin.
    intrinsic: an open3d PinholeCameraIntrinsic (anything with .width, .height and .intrinsic_matrix) or a
    (width, height, fx, fy, cx, cy) tuple.  A hit's depth is its z (the rays are not normalised); among equal depths the
    lowest geometry id, then the lowest triangle index wins; the poses are applied in double precision."""

    def __init__(self, intrinsic, *, device=0):
        import numpy as _np
        if hasattr(intrinsic, "intrinsic_matrix"):
            K = _np.asarray(intrinsic.intrinsic_matrix, dtype=_np.float64).reshape(3, 3)
            cam = (int(intrinsic.width), int(intrinsic.height), K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        else:
            w, h, fx, fy, cx, cy = intrinsic
            cam = (int(w), int(h), float(fx), float(fy), float(cx), float(cy))
        self._cam = cam
        self._device = device
        self._res = None
        self._n = 0

    @staticmethod
    def _mesh(m):
        if isinstance(m, tuple) and len(m) == 2:
            return m
        return (m.vertices, m.triangles)

    def _cast(self, mesh_list, pose_lists, device):
        from . import capi as _capi
        try:
            return _capi.raycast_pinhole([self._mesh(m) for m in mesh_list], pose_lists, self._cam,
                                         self._device if device is None else device)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e

    def cast_rays(self, mesh_list, pose_list, *, device=None):
        """CastRays: True, or False (after the reference's warning) when mesh_list is empty."""
        mesh_list, pose_list = list(mesh_list), list(pose_list)
        if not mesh_list:
            _log_warning("No mesh is provided.")
            return False
        res = self._cast(mesh_list, [pose_list], device)
        self._res = {k: v[0] for k, v in res.items()}
        self._n = len(mesh_list)
        return True

    def cast_rays_batch(self, mesh_list, pose_lists, *, device=None):
        """The same meshes at F lists of poses (the label makers' loop), uploaded once: a dict of (F, H, W) arrays t_hit,
        geometry_ids, primitive_ids and (F, H, W, 3) normals, each frame bit for bit what cast_rays gives.  The getters
        keep describing the last cast_rays call."""
        mesh_list = list(mesh_list)
        if not mesh_list:
            _log_warning("No mesh is provided.")
            return None
        return self._cast(mesh_list, [list(pl) for pl in pose_lists], device)

    def _result(self):
        if self._res is None:
            _log_warning("No ray cast result is available.")
        return self._res

    def get_depth_map(self):
        """(H, W) float32 t_hit, +inf where nothing is hit; an empty array before the first cast"""
        import numpy as _np
        r = self._result()
        return _map_array(r["t_hit"] if r else _np.zeros(0, _np.float32))

    def get_instance_map(self):
        """(H, W) uint32 geometry ids (positions in mesh_list), 0xFFFFFFFF where nothing is hit"""
        import numpy as _np
        r = self._result()
        return _map_array(r["geometry_ids"] if r else _np.zeros(0, _np.uint32))

    def get_primitive_ids(self):
        import numpy as _np
        r = self._result()
        return r["primitive_ids"] if r else _np.zeros(0, _np.uint32)

    def get_normal_map(self):
        import numpy as _np
        r = self._result()
        return r["normals"] if r else _np.zeros((0, 3), _np.float32)

    def _cloud(self, mask):
        import numpy as _np
        W, H, fx, fy, cx, cy = self._cam
        d = _np.empty((H, W, 3), _np.float32)
        d[..., 0] = (((_np.arange(W, dtype=_np.float64) + 0.5) - cx) / fx).astype(_np.float32)[None, :]
        d[..., 1] = (((_np.arange(H, dtype=_np.float64) + 0.5) - cy) / fy).astype(_np.float32)[:, None]
        d[..., 2] = 1.0
        pts = d[mask] * self._res["t_hit"][mask][:, None]   # fp32, as the reference's tensors
        return pts.astype(_np.float64), self._res["normals"][mask].astype(_np.float64)

    def get_point_cloud(self):
        """(points, normals) of the pixels that hit something, in ascending pixel order: rays * t_hit and the primitive normals"""
        import numpy as _np
        if self._result() is None:
            return _np.zeros((0, 3)), _np.zeros((0, 3))
        return self._cloud(_np.isfinite(self._res["t_hit"]))

    def get_instance_point_cloud(self):
        """one (points, normals) per mesh of the last cast: the pixels whose geometry id is that mesh's"""
        if self._result() is None:
            return []
        return [self._cloud(self._res["geometry_ids"] == i) for i in range(self._n)]


class PPFVoting:
    """The two device hot paths of misc3d.pose_estimation.PPFEstimator (src/ppf_estimation.cpp): the point-pair table of a model
    (CalcHashTable, :603-640) and the vote of a scene against it (VotingAndGetPose, :399-524).  points / normals: the ALREADY
    SAMPLED model points with unit normals ((N, 3) arrays, 2 <= N <= 65535); diameter, r_min: what PreprocessTrain derives
    from the model's bounding box.  params: rel_sample_dist (0.05), angle_step (radians, 12 degrees), min_dist_thresh (1/3),
    min_angle_thresh (radians, 30 degrees), faster_mode (True) -- the reference's config fields.  cluster_poses and estimate
    turn the raw poses into ranked, refined results (ClusterPoses, PoseAverage, RefineSparsePose, the centre shift and the
    scoring).  With edge_points / edge_normals (the model's edge points, 1 <= N_e <= 65535, N N_e <= 2^28) the model is
    trained in VotingMode::EdgePoints (Train, :572-593): the table pairs the sample with the edge points, and vote / estimate
    take the scene's edge points as well; pose_estimation.ppf_prepare_scene is PreprocessEstimate, ppf_prepare_model is
    PreprocessTrain, and PPFEstimator puts them together as the reference's class does."""

    def __init__(self, points, normals, diameter, r_min, *, edge_points=None, edge_normals=None, device=0, **params):
        from . import capi as _capi
        try:
            self._model = _capi.PpfModel(points, normals, diameter, r_min, device, edge_points=edge_points, edge_normals=edge_normals,
                                         **params)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e

    @property
    def voting_mode(self):
        """"SampledPoints" or "EdgePoints" (PPFEstimatorConfig::VotingMode)"""
        return "EdgePoints" if self._model.n_edge else "SampledPoints"

    @property
    def centroid(self):
        """the centroid the model was centred by (Train, :551-560): the raw poses are those of the centred model"""
        return self._model.centroid.copy()

    def __len__(self):
        return self._model.n

    def table(self):
        """the flat table: dict(cell_offsets, entry_i, entry_alpha, nbr_offsets, nbr_indices, tmg, centroid, table_size, ...)"""
        from . import capi as _capi
        try:
            return self._model.table()
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e

    def vote(self, scene_points, scene_normals, reference_indices, edge_points=None, edge_normals=None):
        """The reference's pose_list before clustering, in ascending (reference position, model index): poses (K, 4, 4) of the
        centred model, num_votes (K,), corr_mi (K,) -- Pose6D's fields -- and reference (K,), the position in reference_indices
        of the scene point each pose was voted at.  edge_points / edge_normals: the scene's edge points, required on an
        EdgePoints model (the neighbours of a reference point are taken from them) and refused on a SampledPoints one."""
        import numpy as _np

        from . import capi as _capi
        try:
            r = self._model.vote(scene_points, scene_normals, reference_indices, edge_points=edge_points, edge_normals=edge_normals)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e
        return r["poses"], r["votes"].astype(_np.int64), r["model_index"].astype(_np.int64), r["ref_pos"].astype(_np.int64)

    def cluster_poses(self, poses, num_votes, **params):
        """ClusterPoses with PoseAverage (:871-935, :992-1016) of raw poses as vote() returns them.  params: dist_threshold
        (0.05 x diameter), angle_threshold (radians, 12 degrees) and the other fields of m3d_ppf_cluster_params.  -> dict: per valid
        pose (votes descending, ties by input index) order, count_t, label_t, count_r, label_r; min_num_pt_t; per translation
        cluster min_num_pt_r, cluster_votes; per sub-cluster, in (translation cluster, sub-cluster) order, avg_poses (K, 4, 4),
        avg_votes, avg_cluster; stats."""
        from . import capi as _capi
        try:
            return _capi.ppf_cluster_poses(poses, num_votes, device=self._model.device, model=self._model, **params)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e

    def estimate(self, scene_points, scene_normals, reference_indices, edge_points=None, edge_normals=None, **params):
        """Estimate from the vote on (:304-395): vote, cluster, average, refine, shift by the centroid, score.  params: the fields
        of m3d_ppf_cluster_params -- dist_threshold, angle_threshold (radians), ratio (0.6), score_thresh (0.6),
        rel_dist_sparse_thresh (5), num_result (10), refine_method ("NoRefine", "PointToPoint" or "PointToPlane", the default),
        object_id.  edge_points / edge_normals as vote takes them; on an EdgePoints model the refinement still runs against the
        scene sample and the score's expected votes are ratio n n.  -> a list of Pose6D (pose of the UNCENTRED model, q, t,
        num_votes, score, object_id), best first."""
        from . import capi as _capi
        try:
            r = _capi.ppf_estimate(self._model, scene_points, scene_normals, reference_indices, edge_points=edge_points,
                                   edge_normals=edge_normals, **params)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e
        return [Pose6D(r["poses"][k].copy(), r["q"][k].copy(), r["t"][k].copy(), int(r["votes"][k]), float(r["scores"][k]), r["object_id"])
                for k in range(len(r["votes"]))]


def _log_error(msg):
    if int(get_verbosity_level()) >= int(VerbosityLevel.Error):
        print(f"[Misc3D ERROR] {msg}")


class PPFEstimatorConfig:
    """misc3d.pose_estimation.PPFEstimatorConfig (include/misc3d/pose_estimation/ppf_estimation.h, defaults
    src/ppf_estimation.cpp:1392-1405): the reference's fields, nesting, defaults and enum names.  rel_dist_thresh and
    rel_angle_thresh, which the reference's binding forgets, are exposed too."""

    class ReferencePointSelection(_enum.IntEnum):
        Random = 0

    class RefineMethod(_enum.IntEnum):
        NoRefine = 0
        PointToPoint = 1
        PointToPlane = 2

    class VotingMode(_enum.IntEnum):
        SampledPoints = 0
        EdgePoints = 1

    Random = ReferencePointSelection.Random                       # (export_values)
    NoRefine, PointToPoint, PointToPlane = RefineMethod.NoRefine, RefineMethod.PointToPoint, RefineMethod.PointToPlane
    SampledPoints, EdgePoints = VotingMode.SampledPoints, VotingMode.EdgePoints

    class TrainingParam:
        def __init__(self):
            self.invert_model_normal, self.use_external_normal = False, False
            self.rel_sample_dist, self.rel_dense_sample_dist, self.calc_normal_relative = 0.05, 0.025, 0.01

    class ReferenceParam:
        def __init__(self):
            self.method, self.ratio = PPFEstimatorConfig.ReferencePointSelection.Random, 0.6

    class VotingParam:
        def __init__(self):
            import math as _math
            self.method, self.faster_mode = PPFEstimatorConfig.VotingMode.SampledPoints, True
            self.angle_step, self.min_dist_thresh, self.min_angle_thresh = 12.0 / 180.0 * _math.pi, 1.0 / 3, 30.0 / 180.0 * _math.pi

    class EdgeParam:
        def __init__(self):
            self.pts_num = 20

    class RefineParam:
        def __init__(self):
            self.method, self.rel_dist_sparse_thresh = PPFEstimatorConfig.RefineMethod.PointToPlane, 5.0

    def __init__(self):
        import math as _math
        self.training_param, self.ref_param, self.voting_param = self.TrainingParam(), self.ReferenceParam(), self.VotingParam()
        self.edge_param, self.refine_param = self.EdgeParam(), self.RefineParam()
        self.rel_dist_thresh, self.rel_angle_thresh = 0.05, 12.0 / 180.0 * _math.pi
        self.score_thresh, self.num_result, self.object_id = 0.6, 10, 0


class PPFEstimator:
    """misc3d.pose_estimation.PPFEstimator (src/ppf_estimation.cpp: Train :526-601, Estimate :280-397): ppf_prepare_model
    (PreprocessTrain, the contract "PPF model preprocessing" of include/misc3d_amd.h) and a PPFVoting of its sample; then
    ppf_prepare_scene, the reference indices of SampleWithoutDuplicate and PPFVoting.estimate.  Clouds are (N, 3) arrays and come
    back as (points, normals) pairs.  The model's box is rule B1's, not Qhull's: pass the reference's box as
    train(..., bounding_box=(center, extent)) to get the reference's diameter.  dist_threshold = rel_dist_thresh x diameter is
    computed afresh by every train; the reference multiplies its member again on each call (a bug not reproduced)."""

    def __init__(self, config=None, device=0):
        self._device = device
        self._config = PPFEstimatorConfig()
        self._reset()
        if config is not None and not self.set_config(config):
            raise ValueError("PPFEstimator: invalid config")

    def _reset(self):
        import numpy as _np
        e = (_np.zeros((0, 3)), _np.zeros((0, 3)))
        self._voting, self._info, self._diameter, self._dist_threshold, self._poses = None, None, 0.0, 0.0, []
        self._model_sample, self._model_edges, self._scene_sample, self._scene_edges = e, e, e, e

    @staticmethod
    def check_config(config):
        """CheckConfig (:1409-1418)"""
        if config.training_param.rel_dense_sample_dist >= config.training_param.rel_sample_dist:
            _log_error("Dense_sample_dist should be smaller than sample_dist.")
            return False
        return True

    def set_config(self, config):
        if not self.check_config(config):
            return False
        import copy as _copy
        self._config = _copy.deepcopy(config)
        return True

    @property
    def _edge_mode(self):
        return int(self._config.voting_param.method) == int(PPFEstimatorConfig.VotingMode.EdgePoints)

    def train(self, points, normals=None, *, bounding_box=None):
        import numpy as _np

        from . import capi as _capi
        cfg, tp, vp = self._config, self._config.training_param, self._config.voting_param
        self._reset()
        pts = _np.ascontiguousarray(points, dtype=_np.float64).reshape(-1, 3)
        if len(pts) == 0:
            _log_error("There is no input points")
            return False
        bc, be = (None, None) if bounding_box is None else bounding_box
        try:
            m = _capi.ppf_prepare_model(pts, normals, box_center=bc, box_extent=be, device=self._device,
                                        rel_sample_dist=tp.rel_sample_dist, rel_dense_sample_dist=tp.rel_dense_sample_dist if self._edge_mode else 0.0,
                                        calc_normal_relative=tp.calc_normal_relative, invert_model_normal=int(bool(tp.invert_model_normal)),
                                        use_external_normal=int(bool(tp.use_external_normal)), pts_num=int(cfg.edge_param.pts_num))
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e
        info, si = m["info"], m["sample_indices"]
        if len(si) == 0:
            _log_error("There is no input points after preprocessing")
            return False
        sample = (_np.ascontiguousarray(pts[si]), _np.ascontiguousarray(m["normals"][si]))
        edges = (None, None)
        if self._edge_mode:
            if len(m["edge_indices"]) == 0:
                _log_error("Fail to extract edge points!")
                return False
            ei = m["dense_indices"][m["edge_indices"]]
            edges = (_np.ascontiguousarray(pts[ei]), _np.ascontiguousarray(m["normals"][ei]))
        try:
            voting = PPFVoting(sample[0], sample[1], info["diameter"], info["r_min"], edge_points=edges[0], edge_normals=edges[1],
                               device=self._device, rel_sample_dist=tp.rel_sample_dist, angle_step=vp.angle_step,
                               min_dist_thresh=vp.min_dist_thresh, min_angle_thresh=vp.min_angle_thresh, faster_mode=bool(vp.faster_mode))
        except RuntimeError as e:
            # the sample exceeds what PPFVoting accepts (m3d_ppf_model_create's three size refusals); anything else is raised
            if not any(s in str(e) for s in ("ppf: the model must have", "ppf: the table's sort scratch")):
                raise
            _log_error(str(e))
            return False
        self._voting, self._info, self._diameter = voting, info, info["diameter"]
        self._dist_threshold = cfg.rel_dist_thresh * info["diameter"]
        self._model_sample = sample
        if self._edge_mode:
            self._model_edges = edges
        return True

    def estimate(self, points, normals=None, *, seed=None):
        """-> (ret, [Pose6D]).  seed: of the reference points' std::mt19937 (None: drawn from the OS, as std::random_device)"""
        import os as _os

        import numpy as _np

        from . import capi as _capi
        cfg = self._config
        self._poses = []
        if self._voting is None:
            _log_error("Need training before estimating!")
            return False, []
        info = self._info
        try:
            s = _capi.ppf_prepare_scene(points, normals, info["diameter"], cfg.training_param.calc_normal_relative, info["dist_step"],
                                        info["dist_step_dense"] if self._edge_mode else 0.0, int(cfg.edge_param.pts_num), self._device)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e
        self._scene_sample = (s["sample_points"], s["sample_normals"])
        num = len(s["sample_points"])
        if num == 0:
            return False, []
        ep = en = None
        if self._edge_mode:
            if len(s["edge_indices"]) == 0:
                return False, []
            ep = _np.ascontiguousarray(s["dense_points"][s["edge_indices"]])
            en = _np.ascontiguousarray(s["dense_normals"][s["edge_indices"]])
            self._scene_edges = (ep, en)
        if seed is None:
            seed = int.from_bytes(_os.urandom(4), "little")
        ref = _capi.ppf_reference_indices(num, int(cfg.ref_param.ratio * num), seed)
        results = self._voting.estimate(s["sample_points"], s["sample_normals"], ref, edge_points=ep, edge_normals=en,
                                        **self._estimate_params())
        self._poses = results
        return len(results) > 0, results

    def _estimate_params(self):
        cfg = self._config
        return dict(dist_threshold=self._dist_threshold, angle_threshold=cfg.rel_angle_thresh, ratio=cfg.ref_param.ratio,
                    score_thresh=cfg.score_thresh, rel_dist_sparse_thresh=cfg.refine_param.rel_dist_sparse_thresh,
                    num_result=int(cfg.num_result), refine_method=PPFEstimatorConfig.RefineMethod(int(cfg.refine_param.method)).name,
                    object_id=int(cfg.object_id))

    def get_model_diameter(self):
        return self._diameter

    def get_pose(self):
        return list(self._poses)

    getl_pose = get_pose          # (the reference's binding spells it so)

    def get_sampled_model(self):
        return self._model_sample

    def get_sampled_scene(self):
        return self._scene_sample

    def _edges(self, which, what):
        if not self._edge_mode:
            _log_warning(f"Can not get {what} edge points due to edge support is not enabled.")
        return which

    def get_model_edges(self):
        return self._edges(self._model_edges, "model")

    def get_scene_edges(self):
        return self._edges(self._scene_edges, "scene")


class Pose6D:
    """misc3d.pose_estimation.Pose6D's fields (data_structure.h): pose (4, 4), q (w, x, y, z), t, num_votes, score, object_id"""
    __slots__ = ("pose", "q", "t", "num_votes", "score", "object_id")

    def __init__(self, pose, q, t, num_votes, score, object_id):
        self.pose, self.q, self.t, self.num_votes, self.score, self.object_id = pose, q, t, num_votes, score, object_id

    def __repr__(self):
        return f"Pose6D(num_votes={self.num_votes}, score={self.score:.4f}, object_id={self.object_id})"


class _PoseEstimation:
    """misc3d.pose_estimation (python/py_pose_estimation.cpp): RayCastRenderer, PPFEstimator with PPFEstimatorConfig and Pose6D.
    The estimator's stages are here on their own too: its table and its voting in both modes (SampledPoints, EdgePoints), its
    pose clustering, refinement and scoring as PPFVoting, PreprocessEstimate as ppf_prepare_scene, PreprocessTrain as
    ppf_prepare_model and its normal orientation as orient_normals.
    One piece of the reference's PPFEstimator is not part of this build: Open3D's oriented bounding box of Qhull's convex hull.
    The model's box is the PCA box of all points (rule B1 of include/misc3d_amd.h) unless the caller passes one."""
    RayCastRenderer = RayCastRenderer
    PPFVoting = PPFVoting
    PPFEstimator = PPFEstimator
    PPFEstimatorConfig = PPFEstimatorConfig
    Pose6D = Pose6D

    @staticmethod
    def orient_normals(points, normals, radius, seed, device=0):
        """The normal orientation of PreprocessTrain (CalcModelNormalAndSampling, ppf_estimation.cpp:1083-1148) from an already
        oriented seed: signs propagated along the minimum spanning tree of the radius graph (rules O1 - O5 of
        include/misc3d_amd.h).  -> (normals (n, 3), parent (n,) int64: -1 the seed, -2 outside its component, stats dict)"""
        from . import capi as _capi
        try:
            return _capi.orient_normals_mst(points, normals, radius, seed, device)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e

    @staticmethod
    def ppf_prepare_model(points, normals=None, *, box_center=None, box_extent=None, device=0, **params):
        """PPFEstimator::PreprocessTrain (ppf_estimation.cpp:206-241, :1063-1160; rules B1 - B6): the box and what is derived from
        it, normals estimated when None, oriented from the point nearest the view point, the distance-interval samples and the
        dense sample's edge points.  params: rel_sample_dist, rel_dense_sample_dist (<= 0: no dense sample),
        calc_normal_relative, invert_model_normal, use_external_normal, pts_num.  -> dict(normals, sample_indices, dense_indices,
        edge_indices (into the dense sample), info)"""
        from . import capi as _capi
        try:
            return _capi.ppf_prepare_model(points, normals, box_center=box_center, box_extent=box_extent, device=device, **params)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e

    @staticmethod
    def ppf_prepare_scene(points, normals, diameter, calc_normal_relative, dist_step, dist_step_dense=0.0, pts_num=30, device=0):
        """PPFEstimator::PreprocessEstimate (ppf_estimation.cpp:243-278): non-finite points dropped, normals estimated when None
        (Hybrid(calc_normal_relative x diameter, 30)), NormalConsistent, VoxelDownSample(dist_step) and, with dist_step_dense > 0,
        VoxelDownSample(dist_step_dense) with DetectBoundaryPoints(Hybrid(the same radius, pts_num)).  -> dict(sample_points,
        sample_normals, dense_points, dense_normals, edge_indices): the voxel means' normals are not re-normalised."""
        from . import capi as _capi
        try:
            return _capi.ppf_prepare_scene(points, normals, diameter, calc_normal_relative, dist_step, dist_step_dense, pts_num, device)
        except _capi.M3DError as e:
            raise RuntimeError(str(e)) from e


pose_estimation = _PoseEstimation()


def registration_session(*args, **kwargs):
    """capi.RegSession: compute_transformation_ransac cut into begin_chunk / validate / replay, the unit
    misc3d_amd.distributed.registration_ransac_sharded shards over ranks."""
    from . import capi as _capi
    return _capi.RegSession(*args, **kwargs)

__all__ = ["common", "registration", "segmentation", "features", "preprocessing", "reconstruction", "pose_estimation", "registration_icp", "registration_colored_icp", "registration_session", "VerbosityLevel", "set_verbosity_level",
           "get_verbosity_level", "device_count"]
