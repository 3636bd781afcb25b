"""ctypes binding of the C ABI declared in ``include/misc3d_amd.h``.

This is plumbing for the tests, ``bench.py`` and the distributed driver: it loads
``misc3d_amd/lib/libmisc3d_amd.so`` (built in-tree by ``misc3d_amd/csrc/Makefile``) and exposes each
``m3d_*`` entry point with numpy in/out.  It contains no arithmetic and no fallback: if the shared
object is missing, importing fails loudly; if there is no HIP device every compute call raises
``M3DError`` carrying the library's message.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import threading
import os
import sys
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# M3D_FP_ORDER=1|2 in the environment loads the library built for one of the alternative floating-point associations
# (misc3d_amd/csrc/m3d_fp.hpp; tests/test_fp_orders.py runs the parity suite under each); default 0
FP_ORDER = int(os.environ.get("M3D_FP_ORDER", "0") or 0)
# M3D_LIB_VARIANT=<dir>: a diagnostic build under misc3d_amd/lib/<dir>/ (tools/reg_query_fates.sh: -DM3D_REG_TRIP_STATS)
_VARIANT = os.environ.get("M3D_LIB_VARIANT", "")
LIB_PATH = os.path.join(_HERE, "lib", *([_VARIANT] if _VARIANT else ([f"order{FP_ORDER}"] if FP_ORDER else [])), "libmisc3d_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "misc3d_amd.h")

PLANE, SPHERE, CYLINDER = 0, 1, 2
MINIMAL_SAMPLE = {PLANE: 3, SPHERE: 4, CYLINDER: 2}
NUM_PARAMS = {PLANE: 4, SPHERE: 4, CYLINDER: 7}
MODEL_STRIDE = 8

OK, FALSE = 1, 0
ERR_PROBABILITY, ERR_TOO_FEW_POINTS, ERR_NO_NORMALS, ERR_SIZE_MISMATCH = -1, -2, -3, -4
ERR_INVALID_ARG, ERR_DEVICE, ERR_INTERNAL = -5, -6, -7
ERR_NON_FINITE = -8
ERR_CAPACITY = -9


class M3DError(RuntimeError):
    """Raised for negative return codes; mirrors misc3d::LogError -> std::runtime_error
    (src/logging.cpp:64-74), message prefixed like the reference's."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"[Misc3D Error] {msg}")
        self.code = code


class Stats(C.Structure):
    _fields_ = [("fitness", C.c_double), ("inlier_rmse", C.c_double), ("count", C.c_uint64),
                ("iterations", C.c_uint64), ("best_index", C.c_int64), ("general_fit_ok", C.c_int32),
                ("ties", C.c_int32), ("hypotheses_scored", C.c_uint64), ("exact_rmse_evals", C.c_uint64),
                ("ms_sample", C.c_double), ("ms_score", C.c_double), ("ms_refine", C.c_double),
                ("ms_total", C.c_double), ("ms_score_kernel", C.c_double), ("score_launches", C.c_uint32),
                ("early_pick_redone", C.c_uint32), ("pairs_scored", C.c_uint64), ("pairs_exact", C.c_uint64), ("pairs_timed", C.c_uint64)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RegStats(C.Structure):
    _fields_ = [("fitness", C.c_double), ("inlier_rmse", C.c_double), ("validations", C.c_uint64),
                ("iterations", C.c_int64), ("best_index", C.c_int64), ("est_k", C.c_int64),
                ("ms_total", C.c_double), ("ties", C.c_uint64), ("exact_rmse_evals", C.c_uint64),
                ("lds_wave_hypotheses", C.c_uint64), ("global_wave_hypotheses", C.c_uint64),
                ("nn_fp32_screen", C.c_uint64), ("nn_screen_fallbacks", C.c_uint64)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ReplayState(C.Structure):
    _fields_ = [("best_fitness", C.c_double), ("best_rmse", C.c_double), ("best_index", C.c_int64),
                ("best_count", C.c_uint64), ("count", C.c_uint64), ("current_iteration", C.c_uint64),
                ("iterations", C.c_uint64), ("best_rmse_known", C.c_int32), ("stopped", C.c_int32)]


RMSE_FN = C.CFUNCTYPE(C.c_double, C.c_void_p, C.c_size_t)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `make -C misc3d_amd/csrc` (or __graft_entry__.build()); "
                "misc3d_amd has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.m3d_last_error.restype = C.c_char_p
        L.m3d_version.restype = C.c_char_p
        L.m3d_cloud_create.restype = C.c_void_p
        L.m3d_cloud_create.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.m3d_cloud_destroy.argtypes = [C.c_void_p]
        L.m3d_cloud_destroy.restype = None
        L.m3d_host_alloc.restype = C.c_void_p
        L.m3d_host_alloc.argtypes = [C.c_size_t]
        L.m3d_host_free.restype = None
        L.m3d_host_free.argtypes = [C.c_void_p]
        L.m3d_cloud_size.argtypes = [C.c_void_p]
        L.m3d_minimal_fit.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_cloud_size.restype = C.c_size_t
        L.m3d_cloud_fit.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_size_t, C.c_double, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_cloud_score_range.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_size_t, C.c_size_t,
                                            C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_cloud_exact_error.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_cloud_refine.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_cloud_refine_expect.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_int64, C.c_void_p,
                                              C.c_void_p]
        L.m3d_cloud_remove_inliers.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        L.m3d_cloud_original_size.restype = C.c_size_t
        L.m3d_cloud_original_size.argtypes = [C.c_void_p]
        L.m3d_bench_time_score.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_size_t, C.c_int,
                                           C.c_int, C.c_void_p, C.c_void_p]     # include/misc3d_amd_bench.h
        L.m3d_bench_plane_upper_bounds.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_size_t, C.c_void_p]
        L.m3d_bench_upper_bounds.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_size_t, C.c_void_p]
        L.m3d_sampler_create.restype = C.c_void_p
        L.m3d_sampler_create.argtypes = [C.c_size_t, C.c_int, C.c_uint64]
        L.m3d_sampler_destroy.argtypes = [C.c_void_p]
        L.m3d_sampler_destroy.restype = None
        L.m3d_sampler_drawn.argtypes = [C.c_void_p]
        L.m3d_sampler_drawn.restype = C.c_size_t
        L.m3d_sampler_table.argtypes = [C.c_void_p, C.c_size_t]
        L.m3d_sampler_table.restype = C.c_void_p
        L.m3d_cloud_score_shard.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_size_t, C.c_size_t, C.c_size_t,
                                            C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_draw_samples.argtypes = [C.c_size_t, C.c_int, C.c_size_t, C.c_uint64, C.c_void_p]
        L.m3d_replay_init.argtypes = [C.c_void_p]
        L.m3d_replay_init.restype = None
        L.m3d_replay_chunk.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_size_t, C.c_double, C.c_size_t,
                                       C.c_size_t, C.c_void_p, C.c_void_p, RMSE_FN, C.c_void_p]
        L.m3d_replay_chunk.restype = None
        for name in ("m3d_fit_plane", "m3d_fit_sphere"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_size_t, C.c_double, C.c_void_p,
                                         C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_fit_cylinder.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_size_t, C.c_double,
                                       C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_segment_plane_iterative.argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_double,
                                                  C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]
        L.m3d_kabsch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        L.m3d_bench_kabsch_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        L.m3d_bench_icp_sums.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_void_p]
        L.m3d_registration_ransac.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                              C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_double, C.c_double,
                                              C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.m3d_reg_create.restype = C.c_void_p
        L.m3d_reg_create.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_int]
        L.m3d_reg_destroy.restype = None
        L.m3d_reg_destroy.argtypes = [C.c_void_p]
        L.m3d_reg_begin_chunk.argtypes = [C.c_void_p, C.c_void_p]
        L.m3d_reg_validate.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
        L.m3d_reg_replay.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_reg_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_registration_icp.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_int,
                                           C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_registration_icp_plane.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double,
                                                 C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]
        L.m3d_registration_icp_plane_l1.argtypes = L.m3d_registration_icp_plane.argtypes
        L.m3d_multi_scale_icp.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
        L.m3d_color_gradient.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_int, C.c_void_p]
        L.m3d_registration_icp_colored.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_size_t, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_double,
                                                   C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_multi_scale_icp_colored.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double,
                                                  C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_normals_from_map.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_void_p]
        L.m3d_information_matrix.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_void_p]
        L.m3d_detect_boundary_points.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_int, C.c_double,
                                                 C.c_int, C.c_void_p, C.c_void_p]
        L.m3d_farthest_point_sampling.argtypes = [C.c_void_p, C.c_size_t, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
        L.m3d_crop_roi_indices.argtypes = [C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p]
        L.m3d_bench_fps_force_path.argtypes = [C.c_int]
        L.m3d_voxel_down_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_voxel_down_sample_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                  C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]
        L.m3d_bench_voxel_force_path.argtypes = [C.c_int]
        L.m3d_raycast_pinhole.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_double,
                                          C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
        L.m3d_proximity_segment.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_double, C.c_void_p,
                                            C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]
        L.m3d_proximity_segment_nn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_radius_neighbors.argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_size_t, C.c_void_p]
        L.m3d_bench_proximity_cutoffs.argtypes = [C.c_double, C.c_double, C.c_void_p]
        L.m3d_bench_radius_grid_geom.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_bench_reg_grid_k0.argtypes = [C.c_int, C.c_uint64]
        L.m3d_knn_create.restype = C.c_void_p
        L.m3d_knn_create.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        L.m3d_knn_destroy.restype = None
        L.m3d_knn_destroy.argtypes = [C.c_void_p]
        L.m3d_knn_size.restype = C.c_size_t
        L.m3d_knn_size.argtypes = [C.c_void_p]
        L.m3d_knn_dim.argtypes = [C.c_void_p]
        L.m3d_knn_search.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int64, C.c_double, C.c_size_t,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_bench_knn_force_path.argtypes = [C.c_int]
        L.m3d_bench_knn_tile_merge.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int,
                                               C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
        L.m3d_ppf_default_params.restype = None
        L.m3d_ppf_default_params.argtypes = [C.c_void_p]
        L.m3d_ppf_model_create.restype = C.c_void_p
        L.m3d_ppf_model_create.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_void_p]
        L.m3d_ppf_model_destroy.restype = None
        L.m3d_ppf_model_destroy.argtypes = [C.c_void_p]
        L.m3d_ppf_model_size.restype = C.c_size_t
        L.m3d_ppf_model_size.argtypes = [C.c_void_p]
        L.m3d_ppf_model_centroid.argtypes = [C.c_void_p, C.c_void_p]
        L.m3d_ppf_model_table.argtypes = [C.c_void_p] * 8
        L.m3d_ppf_vote.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t] + [C.c_void_p] * 7
        L.m3d_ppf_model_create_edges.restype = C.c_void_p
        L.m3d_ppf_model_create_edges.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_double,
                                                 C.c_void_p, C.c_int, C.c_void_p]
        L.m3d_ppf_model_edge_size.restype = C.c_size_t
        L.m3d_ppf_model_edge_size.argtypes = [C.c_void_p]
        L.m3d_ppf_vote_edges.argtypes = ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                          C.c_size_t, C.c_size_t] + [C.c_void_p] * 7)
        L.m3d_ppf_prepare_scene.argtypes = ([C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_double] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 8)
        L.m3d_orient_normals_mst.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_size_t, C.c_int] + [C.c_void_p] * 3
        L.m3d_ppf_train_params_default_.restype = None
        L.m3d_ppf_train_params_default_.argtypes = [C.c_void_p]
        L.m3d_ppf_prepare_model.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8
        L.m3d_ppf_reference_indices.argtypes = [C.c_size_t, C.c_size_t, C.c_uint32, C.c_void_p]
        L.m3d_bench_ppf_force.argtypes = [C.c_int, C.c_int]
        L.m3d_ppf_default_cluster_params.restype = None
        L.m3d_ppf_default_cluster_params.argtypes = [C.c_void_p, C.c_void_p]
        L.m3d_ppf_cluster_poses.argtypes = ([C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_size_t] + [C.c_void_p] * 6 +
                                            [C.c_size_t] + [C.c_void_p] * 9)
        L.m3d_ppf_estimate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t] + [C.c_void_p] * 7
        L.m3d_ppf_estimate_edges.argtypes = ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                              C.c_size_t, C.c_void_p, C.c_size_t] + [C.c_void_p] * 7)
        L.m3d_bench_ppf_cluster_force.argtypes = [C.c_int]
        L.m3d_bench_scratch_fill.argtypes = [C.c_int]
        L.m3d_bench_scratch_fill_stats.argtypes = [C.c_void_p]
        L.m3d_bench_scratch_probe.argtypes = [C.c_int, C.c_size_t, C.c_void_p]
        L.m3d_estimate_normals.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_void_p]
        L.m3d_compute_fpfh.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p]
        L.m3d_preprocess_fragment.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p]
        L.m3d_bench_fpfh_pair_bins.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.m3d_bench_fpfh_stages.argtypes = ([C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_int, C.c_int] +
                                            [C.c_void_p] * 9)
        L.m3d_match_last_fallbacks.restype = C.c_uint64
        L.m3d_match_last_fallbacks.argtypes = []
        L.m3d_match_mutual_nn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        # multi-GPU: communicators and the sharded entry points
        L.m3d_comm_unique_id.argtypes = [C.c_void_p]
        L.m3d_comm_create_rccl.restype = C.c_void_p
        L.m3d_comm_create_rccl.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.m3d_comm_create_host.restype = C.c_void_p
        L.m3d_comm_create_host.argtypes = [C.c_int, C.c_int, ALLGATHER_FN, C.c_void_p]
        L.m3d_comm_create_local.argtypes = [C.c_int, C.c_void_p]
        L.m3d_comm_destroy.restype = None
        L.m3d_comm_destroy.argtypes = [C.c_void_p]
        L.m3d_comm_world.argtypes = [C.c_void_p]
        L.m3d_comm_rank.argtypes = [C.c_void_p]
        L.m3d_comm_collectives.restype = C.c_uint64
        L.m3d_comm_collectives.argtypes = [C.c_void_p]
        L.m3d_cloud_fit_sharded.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_size_t, C.c_double, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_segment_plane_iterative_clouds.argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_double,
                                                          C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_segment_plane_iterative_sharded.argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_double,
                                                          C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_segment_plane_iterative_multi.argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_double,
                                                        C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_fit_multi.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_size_t, C.c_double,
                                    C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.m3d_registration_ransac_sharded.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                                      C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_double,
                                                      C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                      C.c_void_p]
        L.m3d_bench_fp64_issue_rate.argtypes = [C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        L.m3d_bench_cloud_setup_ms.argtypes = [C.c_void_p, C.c_void_p]
        L.m3d_bench_last_segment_ms.argtypes = [C.c_void_p]
        L.m3d_bench_reg_checkers.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double]
        L.m3d_get_config.restype = None
        L.m3d_get_config.argtypes = [C.c_void_p]
        L.m3d_set_config.argtypes = [C.c_void_p]
        L.m3d_release_cached.restype = None
        L.m3d_release_cached.argtypes = [C.c_int]
        _lib = L
    return _lib


class Config(C.Structure):
    """m3d_config (include/misc3d_amd.h): the library's tunables."""
    _fields_ = [(k, C.c_int32) for k in ("dense_scoring", "speculative_refine", "lead_hypotheses",
                                         "score_groups_per_block", "score_min_workgroups", "dense_workgroups",
                                         "reg_neighbour_lists", "reg_prune", "match_brute", "match_fp32_screen",
                                         "pool_limit_mb", "kernel_timing", "reg_sorted_lists", "score_fp32_screen",
                                         "cull_fp32", "reg_fp32_screen", "sorted_tombstones", "score_mfma", "score_mfma_groups", "score_waves4", "score_waves4_groups", "score_phases", "compact_one_pass", "plane_bound",
                                         "lanes", "wait_spin_us", "prestream", "chunk_cap", "first_chunk", "reg_cells_per_radius", "match_pipeline", "reg_cache", "device_aliases", "lanes_eager", "list_mask", "mask_early", "ref_bound")]


def fp64_issue_rate(device=0, ms_target=2.0):
    """m3d_bench_fp64_issue_rate (include/misc3d_amd_bench.h) -> (1e12 fp64 lane-ops/s the device sustains, ms measured)"""
    t, ms = C.c_double(0), C.c_double(0)
    _check(lib().m3d_bench_fp64_issue_rate(device, ms_target, C.cast(C.byref(t), C.c_void_p), C.cast(C.byref(ms), C.c_void_p)))
    return float(t.value), float(ms.value)


def match_last_path() -> int:
    """m3d_bench_match_last_path: bit 0 MFMA screen, 1 sliced uploads, 2 redone whole, 3 fp32 screen, 4 brute force (the calling thread's last match)"""
    f = lib().m3d_bench_match_last_path
    f.restype = C.c_uint
    f.argtypes = []
    return int(f())


def get_config() -> Config:
    c = Config()
    lib().m3d_get_config(C.byref(c))
    return c


def set_config(**kw) -> Config:
    """Change some tunables (m3d_set_config); returns the PREVIOUS settings, to be restored with restore_config."""
    old = get_config()
    new = get_config()
    for k, v in kw.items():
        if not hasattr(new, k):
            raise AttributeError(k)
        setattr(new, k, int(v))
    _check(lib().m3d_set_config(C.byref(new)))
    return old


def restore_config(cfg: Config):
    _check(lib().m3d_set_config(C.byref(cfg)))


class Comm:
    """m3d_comm: the exchange of the hypothesis-sharded entry points (include/misc3d_amd.h).

    Comm.rccl(group, device)   one process per GPU: rank 0's ncclUniqueId travels over `group` (any
                               torch.distributed group, e.g. gloo), then ncclCommInitRank inside the library.
    Comm.host(world, rank, fn) fn(send: bytes) -> bytes of world * len(send): caller-supplied all-gather.
    Comm.torch_host(group)     the same over torch.distributed.all_gather_into_tensor of `group` (tests: gloo)."""

    def __init__(self, handle, keep=None):
        if not handle:
            raise M3DError(ERR_DEVICE, last_error())
        self._h = handle
        self._keep = keep

    @classmethod
    def rccl(cls, group=None, device=0, world=None, rank=None):
        import torch
        import torch.distributed as dist
        if world is None:
            world, rank = (dist.get_world_size(group), dist.get_rank(group)) if dist.is_initialized() else (1, 0)
        ident = np.zeros(128, dtype=np.uint8)
        status = np.zeros(129, dtype=np.uint8)     # the id + one byte that says rank 0 got one (nobody waits for a rank that raised)
        err = None
        if rank == 0:
            try:
                _check(lib().m3d_comm_unique_id(_p(ident)))
                status[:128] = ident
                status[128] = 1
            except M3DError as e:
                err = e
        if world > 1:
            t = torch.from_numpy(status)
            dist.broadcast(t, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        if not status[128]:
            raise err if err is not None else M3DError(-6, "rank 0 could not create an RCCL unique id")
        ident = np.ascontiguousarray(status[:128])
        # librccl prints a version banner to STDOUT on its first communicator; callers (bench.py) own stdout, so the
        # banner is sent to stderr: fd 1 points at fd 2 for the duration of the call, C stdio flushed on both sides.
        # SIDE EFFECT: the redirection is process-wide and not thread-safe -- whatever another thread writes
        # to stdout while ncclCommInitRank runs (it can take seconds) lands on stderr; M3D_RCCL_KEEP_STDOUT=1 skips it
        # (the banner then goes where librccl sends it)
        libc = C.CDLL(None)
        sys.stdout.flush()
        libc.fflush(None)
        if os.environ.get("M3D_RCCL_KEEP_STDOUT") == "1":
            return cls(lib().m3d_comm_create_rccl(_p(ident), world, rank, device))
        saved = os.dup(1)
        os.dup2(2, 1)
        try:
            h = lib().m3d_comm_create_rccl(_p(ident), world, rank, device)
        finally:
            libc.fflush(None)
            os.dup2(saved, 1)
            os.close(saved)
        return cls(h)

    @classmethod
    def host(cls, world, rank, fn):
        def _cb(_user, send, recv, nbytes):
            try:
                out = fn(C.string_at(send, nbytes))
                if len(out) != nbytes * world:
                    return 2
                C.memmove(recv, out, nbytes * world)
                return 0
            except Exception:       # noqa: BLE001 -- must not unwind through the C frame
                import traceback
                traceback.print_exc()
                return 1
        cb = ALLGATHER_FN(_cb)
        return cls(lib().m3d_comm_create_host(world, rank, cb, None), keep=cb)

    @classmethod
    def torch_host(cls, group=None):
        import torch
        import torch.distributed as dist
        world, rank = dist.get_world_size(group), dist.get_rank(group)

        def gather(b):
            t = torch.frombuffer(bytearray(b), dtype=torch.uint8)
            out = torch.empty(world * len(b), dtype=torch.uint8)
            dist.all_gather_into_tensor(out, t, group=group)
            return out.numpy().tobytes()
        return cls.host(world, rank, gather)

    @property
    def world(self):
        return int(lib().m3d_comm_world(self._h))

    @property
    def rank(self):
        return int(lib().m3d_comm_rank(self._h))

    @property
    def collectives(self):
        return int(lib().m3d_comm_collectives(self._h))

    def close(self):
        if getattr(self, "_h", None):
            lib().m3d_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def last_error() -> str:
    return lib().m3d_last_error().decode()


def device_count() -> int:
    return int(lib().m3d_device_count())


def _check(rc: int) -> int:
    if rc < 0:
        raise M3DError(rc, last_error())
    return rc


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _addr(a):
    """address of a (contiguous) array for a c_void_p parameter, or None"""
    return a.__array_interface__["data"][0] if a is not None else None


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _seed_ref(seed):
    if seed is None:
        return None, None
    s = C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    return s, C.byref(s)


class Fit:
    """ret: 1 = reference `true`, 0 = reference `false`; params: best model AFTER RefineModel (not zeroed; callers zero on
    ret == 0); inliers: uint64, ascending; stats: m3d_stats as a dict (+ "n_inliers"), built when first asked for."""
    __slots__ = ("ret", "params", "inliers", "_stats", "_raw")

    def __init__(self, ret, params, inliers, stats):
        self.ret = ret
        self.params = params
        self.inliers = inliers
        if isinstance(stats, dict):
            self._stats, self._raw = stats, None
        else:   # (Stats structure, inlier count)
            self._stats, self._raw = None, stats

    @property
    def stats(self) -> dict:
        if self._stats is None:
            st, ni = self._raw
            self._stats = st.asdict()
            self._stats["n_inliers"] = int(ni)
            self._raw = None
        return self._stats

    def __iter__(self):   # (ret, params, inliers, stats), as the dataclass this used to be unpacked
        return iter((self.ret, self.params, self.inliers, self.stats))


class Sampler:
    """m3d_sampler: the sequential RandomSampler (utils.h:71-97) with an explicit seed; records its table."""

    def __init__(self, n_points, kind, seed):
        self.kind = kind
        self.m = MINIMAL_SAMPLE[kind]
        self._h = lib().m3d_sampler_create(n_points, kind, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF))
        if not self._h:
            raise M3DError(ERR_INVALID_ARG, last_error())

    def table(self, n_hyp):
        """(n_hyp, m) uint32 view of the first n_hyp samples (drawing them if necessary)."""
        ptr = lib().m3d_sampler_table(self._h, n_hyp)
        if n_hyp == 0:
            return np.zeros((0, self.m), dtype=np.uint32)
        buf = (C.c_uint32 * (n_hyp * self.m)).from_address(ptr)
        return np.frombuffer(buf, dtype=np.uint32).reshape(n_hyp, self.m)

    @property
    def drawn(self):
        return int(lib().m3d_sampler_drawn(self._h))

    def close(self):
        if getattr(self, "_h", None):
            lib().m3d_sampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_layout(begin, end, slice_, world):
    """Index bookkeeping of m3d_cloud_score_shard: for the window [begin, end) cut into slices of
    `slice_`, returns (mine, order) where mine[r] = global indices owned by rank r (ascending) and the
    global order is recovered from the rank-major concatenation (padded to max_mine per rank) through
    `order`: global_records = gathered.reshape(world, max_mine)[order_rank, order_pos]."""
    g = np.arange(begin, end, dtype=np.int64)
    j = (g - begin) // slice_
    owner = (j % world).astype(np.int64)
    pos = np.empty(len(g), dtype=np.int64)
    counts = np.zeros(world, dtype=np.int64)
    for r in range(world):
        sel = owner == r
        k = int(sel.sum())
        pos[sel] = np.arange(k)
        counts[r] = k
    return owner, pos, counts


class _PinnedU64:
    """n uint64 of page-locked host memory from m3d_host_alloc, exposed through the array interface so that numpy
    arrays made from it (and their views) keep it alive."""

    def __init__(self, n):
        self._ptr = lib().m3d_host_alloc(8 * n)
        if not self._ptr:
            raise MemoryError(last_error())
        self.__array_interface__ = {"shape": (n,), "typestr": "<u8", "data": (self._ptr, False), "version": 3}

    def __del__(self):
        try:
            if self._ptr:
                lib().m3d_host_free(self._ptr)
                self._ptr = None
        except Exception:
            pass


class Cloud:
    """Resident SoA copy of a point cloud in HBM (RANSAC::SetPointCloud, ransac.h:469-475)."""

    def make_sampler(self, kind, seed):
        return Sampler(self.n, kind, seed)

    def score_shard_packed(self, sampler, threshold, begin, end, slice_, world, rank):
        """m3d_cloud_score_shard with valid == NULL -> uint32 records (valid << 31 | count) of this rank's hypotheses."""
        rec = np.empty(max(end - begin, 1), dtype=np.uint32)
        n = C.c_size_t(0)
        _check(lib().m3d_cloud_score_shard(self._h, sampler._h, threshold, begin, end, slice_, world, rank, _p(rec),
                                           None, C.cast(C.byref(n), C.c_void_p)))
        return rec[: n.value]

    def score_shard(self, sampler, threshold, begin, end, slice_, world, rank):
        """m3d_cloud_score_shard -> (valid, counts) of this rank's hypotheses in [begin, end)."""
        cap = end - begin
        cnt = np.empty(max(cap, 1), dtype=np.uint32)
        val = np.empty(max(cap, 1), dtype=np.uint8)
        n = C.c_size_t(0)
        _check(lib().m3d_cloud_score_shard(self._h, sampler._h, threshold, begin, end, slice_, world, rank, _p(cnt),
                                           _p(val), C.cast(C.byref(n), C.c_void_p)))
        return val[: n.value], cnt[: n.value]

    def __init__(self, xyz, normals=None, device: int = 0, lane: int = -1):
        """lane >= 0: m3d_cloud_create_lane -- the cloud lives on THAT lane of the device (a single-threaded caller spreads its
        clouds over the lanes so that fit_batch can run their fits side by side); -1: the calling thread's own lane."""
        xyz = _f64(xyz).reshape(-1, 3)
        nrm = _f64(normals).reshape(-1, 3) if normals is not None else None
        if nrm is not None and len(nrm) != len(xyz):
            raise ValueError("normals and points differ in length")
        self.n = len(xyz)            # points currently in the cloud (shrinks with remove_inliers)
        self.n_created = len(xyz)    # index lists refer to the cloud as created
        self._host_xyz, self._host_nrm = xyz, nrm     # for minimal_model (host-side MinimalFit of one sample)
        if lane >= 0:
            f = lib().m3d_cloud_create_lane
            f.restype = C.c_void_p
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
            self._h = f(_p(xyz), _p(nrm), self.n, device, int(lane))
        else:
            self._h = lib().m3d_cloud_create(_p(xyz), _p(nrm), self.n, device)
        if not self._h:
            raise M3DError(ERR_DEVICE, last_error())

    def setup_ms(self):
        """m3d_bench_cloud_setup_ms -> dict(total, upload_transpose, bbox, sort, tile_boxes) in ms (the phases are filled
        when m3d_config.kernel_timing was set at creation)."""
        out = np.zeros(5)
        _check(lib().m3d_bench_cloud_setup_ms(self._h, _p(out)))
        return dict(zip(("total", "upload_transpose", "bbox", "sort", "tile_boxes"), (float(v) for v in out)))

    def _out_buf(self):
        """Per-cloud index-list buffer (n_created uint64), page-locked through m3d_host_alloc when possible: the
        library then copies the inlier list while the GeneralFit sums run (include/misc3d_amd.h).  The block is
        owned by the array (and every view of it, e.g. fit(copy=False).inliers): it is released when the last
        one goes away, not by close()."""
        if getattr(self, "_inl_buf", None) is None:
            n = max(self.n_created, 1)
            try:
                self._inl_buf = np.asarray(_PinnedU64(n))
            except MemoryError:
                self._inl_buf = np.empty(n, dtype=np.uint64)
        return self._inl_buf

    def close(self):
        if getattr(self, "_h", None):
            lib().m3d_cloud_destroy(self._h)
            self._h = None
        self._inl_buf = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def fit(self, kind, threshold=0.01, max_iteration=1000, probability=0.9999, seed=None,
            want_inliers=True, copy=True) -> Fit:
        """m3d_cloud_fit.  copy=False returns a view of a per-Cloud output buffer that the next
        call overwrites (the C ABI writes into caller-allocated memory; this avoids re-allocating
        8 bytes x N per call)."""
        params = np.zeros(NUM_PARAMS[kind])
        inl = None
        if want_inliers:
            # copy=True: the list is copied out anyway -- the thread's page-locked scratch serves every cloud (a buffer per
            # cloud costs a hipHostMalloc of 8 bytes x N: 14 ms for 10 M points, paid by the first fit on it)
            inl = _seg_scratch(max(self.n_created, 1)) if copy else None
            if inl is None:
                inl = self._out_buf()
        ni = C.c_size_t(0)
        st = Stats()
        _s, sref = _seed_ref(seed)
        # (byref objects and plain addresses go straight into c_void_p parameters: ndarray.ctypes.data_as and ctypes.cast
        #  cost 2.4 and 0.7 us apiece, a third of this wrapper's time around a 0.27 ms fit)
        rc = _check(lib().m3d_cloud_fit(self._h, kind, threshold, max_iteration, probability, sref, _addr(params),
                                        _addr(inl), C.byref(ni), C.byref(st)))
        if want_inliers:
            inliers = inl[: ni.value].copy() if copy else inl[: ni.value]
        else:
            inliers = np.zeros(0, dtype=np.uint64)
        return Fit(rc, params, inliers, (st, ni.value))

    def fit_sharded(self, comm, kind, threshold=0.01, max_iteration=1000, probability=0.9999, seed=None,
                    want_inliers=True, copy=True) -> Fit:
        """m3d_cloud_fit_sharded: the same fit with the hypothesis loop sharded over the ranks of `comm` (every
        rank calls it on its own replica of the cloud and gets the same result)."""
        params = np.zeros(NUM_PARAMS[kind])
        inl = self._out_buf() if want_inliers else None
        ni = C.c_size_t(0)
        st = Stats()
        _s, sref = _seed_ref(seed)
        rc = _check(lib().m3d_cloud_fit_sharded(self._h, comm._h if comm is not None else None, kind, threshold,
                                                max_iteration, probability, sref, _addr(params), _addr(inl),
                                                C.byref(ni), C.byref(st)))
        if want_inliers:
            inliers = inl[: ni.value].copy() if copy else inl[: ni.value]
        else:
            inliers = np.zeros(0, dtype=np.uint64)
        return Fit(rc, params, inliers, (st, ni.value))

    def score_range(self, kind, threshold, samples, begin=0, end=None, want_models=True):
        """m3d_cloud_score_range -> (valid, models or None, counts) for hypotheses [begin, end)."""
        samples = np.ascontiguousarray(samples, dtype=np.uint32).reshape(-1, MINIMAL_SAMPLE[kind])
        end = len(samples) if end is None else end
        cnt = np.empty(end - begin, dtype=np.uint32)
        val = np.empty(end - begin, dtype=np.uint8)
        mod = np.empty((end - begin, MODEL_STRIDE)) if want_models else None
        _check(lib().m3d_cloud_score_range(self._h, kind, threshold, _p(samples), begin, end, _p(cnt), _p(val),
                                           _p(mod)))
        return val, (mod[:, : NUM_PARAMS[kind]].copy() if want_models else None), cnt

    def time_score(self, kind, threshold, samples, reps=5, mode=0):
        """(average ms per launch over `reps` launches measured with HIP events, surviving
        (tile, hypothesis) pairs).  mode 0 = score_list_k, 1 = cull_k, 2 = dense score_k."""
        samples = np.ascontiguousarray(samples, dtype=np.uint32).reshape(-1, MINIMAL_SAMPLE[kind])
        ms = C.c_double(0)
        listed = C.c_uint64(0)
        _check(lib().m3d_bench_time_score(self._h, kind, threshold, _p(samples), len(samples), reps, mode,
                                          C.cast(C.byref(ms), C.c_void_p), C.cast(C.byref(listed), C.c_void_p)))
        return float(ms.value), int(listed.value)

    def plane_upper_bounds(self, threshold, samples):
        """m3d_bench_plane_upper_bounds -> uint32 upper bound of every plane hypothesis' inlier count (plane_bound_k, nothing pruned)"""
        samples = np.ascontiguousarray(samples, dtype=np.uint32).reshape(-1, 3)
        ub = np.zeros(len(samples), dtype=np.uint32)
        _check(lib().m3d_bench_plane_upper_bounds(self._h, threshold, _p(samples), len(samples), _p(ub)))
        return ub

    def plane_ref_upper_bounds(self, threshold, samples, ref_index):
        """m3d_bench_plane_ref_upper_bounds -> uint32 upper bounds from the histograms along hypothesis ref_index's plane alone"""
        samples = np.ascontiguousarray(samples, dtype=np.uint32).reshape(-1, 3)
        ub = np.zeros(len(samples), dtype=np.uint32)
        f = lib().m3d_bench_plane_ref_upper_bounds
        f.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
        _check(f(self._h, threshold, _p(samples), len(samples), int(ref_index), _p(ub)))
        return ub

    def upper_bounds(self, kind, threshold, samples):
        """m3d_bench_upper_bounds -> uint32 upper bound of every hypothesis' inlier count (plane_bound_k<kind>, nothing pruned)"""
        samples = np.ascontiguousarray(samples, dtype=np.uint32).reshape(-1, MINIMAL_SAMPLE[kind])
        ub = np.zeros(len(samples), dtype=np.uint32)
        _check(lib().m3d_bench_upper_bounds(self._h, kind, threshold, _p(samples), len(samples), _p(ub)))
        return ub

    def exact_error(self, kind, threshold, model):
        model = _f64(model)
        cnt = C.c_uint64(0)
        err = C.c_double(0)
        _check(lib().m3d_cloud_exact_error(self._h, kind, threshold, _p(model), C.cast(C.byref(cnt), C.c_void_p),
                                           C.cast(C.byref(err), C.c_void_p)))
        return int(cnt.value), float(err.value)

    refine_takes_expected = True

    def refine(self, kind, threshold, params, copy=True, expected=None):
        """m3d_cloud_refine; expected = inlier count already known from the scoring records (m3d_cloud_refine_expect)"""
        params = _f64(params).copy()
        inl = self._out_buf()
        ni = C.c_size_t(0)
        rc = _check(lib().m3d_cloud_refine_expect(self._h, kind, threshold, _p(params),
                                                  -1 if expected is None else int(expected), _p(inl),
                                                  C.cast(C.byref(ni), C.c_void_p)))
        return rc, params, (inl[: ni.value].copy() if copy else inl[: ni.value])

    def minimal_model(self, kind, threshold, sample_row):
        """MinimalFit of ONE sample -> 8-double model record.  Host-side (m3d_minimal_fit, bit-identical to the
        device) while the cloud is as created; after remove_inliers the sample indexes the shrunk device
        cloud, so the one-row device launch is used."""
        row = np.ascontiguousarray(sample_row, dtype=np.uint32).reshape(-1)
        if self.n == self.n_created:
            pts = np.ascontiguousarray(self._host_xyz[row])
            nrm = np.ascontiguousarray(self._host_nrm[row]) if self._host_nrm is not None else None
            model = np.zeros(8)
            ok = C.c_uint8(0)
            _check(lib().m3d_minimal_fit(kind, _p(pts), _p(nrm), _p(model), C.cast(C.byref(ok), C.c_void_p)))
            return model[: NUM_PARAMS[kind]].copy()
        _, mod, _ = self.score_range(kind, threshold, row.reshape(1, -1), 0, 1)
        return mod[0]

    def remove_inliers(self, kind, threshold, model):
        """m3d_cloud_remove_inliers: SelectByIndex(inliers of `model`, invert=True) in place -> #removed."""
        model = _f64(model).copy()
        nr = C.c_size_t(0)
        _check(lib().m3d_cloud_remove_inliers(self._h, kind, threshold, _p(model), C.cast(C.byref(nr), C.c_void_p)))
        self.n = int(lib().m3d_cloud_size(self._h))
        return nr.value


def draw_samples(n_points, kind, n_hyp, seed):
    out = np.zeros((n_hyp, MINIMAL_SAMPLE[kind]), dtype=np.uint32)
    _check(lib().m3d_draw_samples(n_points, kind, n_hyp, C.c_uint64(seed), _p(out)))
    return out


def fit(kind, xyz, normals=None, threshold=0.01, max_iteration=1000, probability=0.9999, seed=None,
        device=0, copy=True) -> Fit:
    """One-shot m3d_fit_plane / m3d_fit_sphere / m3d_fit_cylinder.  copy=False: the inlier list is a view of the
    thread's page-locked scratch (overwritten by the next call)."""
    xyz = _f64(xyz).reshape(-1, 3)
    n = len(xyz)
    params = np.zeros(NUM_PARAMS[kind])
    # filled by the library up to n_inliers, copied out below: the thread's page-locked scratch when there is one (the
    # compaction kernel then stores the index list straight into it)
    inl = _seg_scratch(max(n, 1))
    if inl is None:
        inl = np.empty(max(n, 1), dtype=np.uint64)
    ni = C.c_size_t(0)
    st = Stats()
    _s, sref = _seed_ref(seed)
    sp = C.cast(sref, C.c_void_p) if sref else None
    nip, stp = C.cast(C.byref(ni), C.c_void_p), C.cast(C.byref(st), C.c_void_p)
    if kind == CYLINDER:
        nrm = _f64(normals).reshape(-1, 3) if normals is not None else None
        rc = lib().m3d_fit_cylinder(_p(xyz), _p(nrm), n, threshold, max_iteration, probability, sp, device,
                                    _p(params), _p(inl), nip, stp)
    else:
        fn = lib().m3d_fit_plane if kind == PLANE else lib().m3d_fit_sphere
        rc = fn(_p(xyz), n, threshold, max_iteration, probability, sp, device, _p(params), _p(inl), nip, stp)
    _check(rc)
    d = st.asdict()
    d["n_inliers"] = int(ni.value)
    return Fit(rc, params, inl[: ni.value].copy() if copy else inl[: ni.value], d)


_seg_tls = threading.local()
_SEG_SCRATCH_MAX = 1 << 25      # uint64 entries (256 MB): larger clouds take the pageable path


def _seg_scratch(n):
    """n uint64 of page-locked scratch, kept per thread and grown on demand (None: too large, or pinning failed)."""
    if n > _SEG_SCRATCH_MAX:
        return None
    buf = getattr(_seg_tls, "buf", None)
    if buf is None or len(buf) < n:
        try:
            buf = np.asarray(_PinnedU64(n))
        except MemoryError:
            return None
        _seg_tls.buf = buf
    return buf[:n]


def segment_plane_iterative(xyz, threshold, max_iteration=100, min_ratio=0.05, seed=None, device=0,
                            max_clusters=4096, copy=True, with_points=False):
    """m3d_segment_plane_iterative (with_points: m3d_segment_plane_iterative_clouds -- a fourth return value, the list of
    the clusters' (count, 3) point arrays, views of one array gathered on the device).  copy=True (default): the library writes the index lists into a page-locked scratch
    the binding keeps per thread, every cluster is returned as an array of its own.  copy=False returns the clusters as
    views of ONE pageable index array instead (no copies, but the library then reaches the array through staged copies
    and fresh pages: on 10 M points 43 ms against 37)."""
    xyz = _f64(xyz).reshape(-1, 3)
    n = len(xyz)
    planes = np.zeros((max_clusters, 4))
    offs = np.zeros(max_clusters + 1, dtype=np.uint64)
    # filled by the library up to the last offset.  copy=True: the clusters are copied out anyway, so the library may as
    # well write into a page-locked scratch kept per thread (its kernels then store the index lists straight into it: no
    # staged copies into fresh pageable pages, which on 10 M points cost 3 ms of page faults and a blocking copy per round)
    idx = _seg_scratch(max(n, 1)) if copy else None
    if idx is None:
        idx = np.empty(max(n, 1), dtype=np.uint64)
    k = C.c_size_t(0)
    _s, sref = _seed_ref(seed)
    if with_points:
        cpts = np.empty((max(n, 1), 3))
        rc = _check(lib().m3d_segment_plane_iterative_clouds(_p(xyz), n, threshold, max_iteration, min_ratio,
                                                             C.cast(sref, C.c_void_p) if sref else None, device,
                                                             max_clusters, _p(planes), _p(offs), _p(idx), _p(cpts),
                                                             C.cast(C.byref(k), C.c_void_p)))
    else:
        rc = _check(lib().m3d_segment_plane_iterative(_p(xyz), n, threshold, max_iteration, min_ratio,
                                                      C.cast(sref, C.c_void_p) if sref else None, device, max_clusters,
                                                      _p(planes), _p(offs), _p(idx), C.cast(C.byref(k), C.c_void_p)))
    k = k.value
    clusters = [idx[int(offs[i]): int(offs[i + 1])].copy() if copy else idx[int(offs[i]): int(offs[i + 1])] for i in range(k)]
    if with_points:
        return rc, planes[:k].copy(), clusters, [cpts[int(offs[i]): int(offs[i + 1])] for i in range(k)]
    return rc, planes[:k].copy(), clusters


def last_segment_ms():
    """m3d_bench_last_segment_ms -> dict of the calling thread's last segmentation call (ms)"""
    out = np.zeros(6)
    _check(lib().m3d_bench_last_segment_ms(_p(out)))
    return {"total": out[0], "cloud_create": out[1], "rounds": out[2], "final_copy": out[3], "big_rounds": out[4],
            "n_big_rounds": int(out[5]), "n_rounds": int(round((out[5] - int(out[5])) * 1e4))}


def segment_plane_iterative_sharded(xyz, comm, threshold, max_iteration=100, min_ratio=0.05, seed=None, device=0,
                                    max_clusters=4096):
    """m3d_segment_plane_iterative_sharded (every rank of `comm` calls it with the same cloud)."""
    xyz = _f64(xyz).reshape(-1, 3)
    n = len(xyz)
    planes = np.zeros((max_clusters, 4))
    offs = np.zeros(max_clusters + 1, dtype=np.uint64)
    idx = np.empty(max(n, 1), dtype=np.uint64)
    k = C.c_size_t(0)
    _s, sref = _seed_ref(seed)
    rc = _check(lib().m3d_segment_plane_iterative_sharded(_p(xyz), n, threshold, max_iteration, min_ratio,
                                                          C.cast(sref, C.c_void_p) if sref else None, device,
                                                          comm._h if comm is not None else None, max_clusters,
                                                          _p(planes), _p(offs), _p(idx), C.cast(C.byref(k), C.c_void_p)))
    k = k.value
    return rc, planes[:k].copy(), [idx[int(offs[i]): int(offs[i + 1])].copy() for i in range(k)]


def segment_plane_iterative_multi(xyz, devices, threshold, max_iteration=100, min_ratio=0.05, seed=None,
                                  max_clusters=4096):
    """m3d_segment_plane_iterative_multi: one process, a thread and a replica per device of `devices`."""
    xyz = _f64(xyz).reshape(-1, 3)
    n = len(xyz)
    dev = np.ascontiguousarray(devices, dtype=np.int32)
    planes = np.zeros((max_clusters, 4))
    offs = np.zeros(max_clusters + 1, dtype=np.uint64)
    idx = np.empty(max(n, 1), dtype=np.uint64)
    k = C.c_size_t(0)
    _s, sref = _seed_ref(seed)
    rc = _check(lib().m3d_segment_plane_iterative_multi(_p(xyz), n, threshold, max_iteration, min_ratio,
                                                        C.cast(sref, C.c_void_p) if sref else None, _p(dev), len(dev),
                                                        max_clusters, _p(planes), _p(offs), _p(idx),
                                                        C.cast(C.byref(k), C.c_void_p)))
    k = k.value
    return rc, planes[:k].copy(), [idx[int(offs[i]): int(offs[i + 1])].copy() for i in range(k)]


class FitJob(C.Structure):
    """m3d_fit_job (include/misc3d_amd.h)"""
    _fields_ = [("cloud", C.c_void_p), ("kind", C.c_int32), ("has_seed", C.c_int32), ("threshold", C.c_double),
                ("probability", C.c_double), ("max_iteration", C.c_uint64), ("seed", C.c_uint64), ("inliers", C.c_void_p),
                ("params", C.c_double * 8), ("n_inliers", C.c_uint64), ("rc", C.c_int32), ("reserved_", C.c_int32), ("stats", Stats)]


def fit_batch(jobs, inflight=0, want_inliers=True):
    """m3d_cloud_fit_batch: jobs = [(cloud, kind, threshold, max_iteration, probability, seed), ...] -> [Fit, ...] in the order
    given.  ONE call into the library (one release of the interpreter's lock): the jobs of a cloud run in order, clouds on
    different lanes (Cloud(..., lane=k)) or devices side by side."""
    n = len(jobs)
    if n == 0:
        return []
    arr = (FitJob * n)()
    bufs = []
    for k, (cloud, kind, thr, it, prob, seed) in enumerate(jobs):
        j = arr[k]
        j.cloud, j.kind, j.threshold, j.max_iteration, j.probability = cloud._h, int(kind), float(thr), int(it), float(prob)
        if seed is not None:
            j.seed, j.has_seed = int(seed) & 0xFFFFFFFFFFFFFFFF, 1
        if want_inliers:
            b = np.empty(max(cloud.n_created, 1), dtype=np.uint64)      # (one list per job: they are all alive at the end)
            bufs.append(b)
            j.inliers = b.ctypes.data
        else:
            bufs.append(None)
    f = lib().m3d_cloud_fit_batch
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    _check(f(C.cast(arr, C.c_void_p), n, int(inflight)))
    out = []
    for k in range(n):
        j = arr[k]
        inl = bufs[k][: j.n_inliers] if want_inliers else np.zeros(0, dtype=np.uint64)
        st = j.stats.asdict()
        st["n_inliers"] = int(j.n_inliers)
        out.append(Fit(int(j.rc), np.array(j.params[: NUM_PARAMS[int(j.kind)]]), inl, st))
    return out


def fit_multi(kind, xyz, devices, normals=None, threshold=0.01, max_iteration=1000, probability=0.9999, seed=None) -> Fit:
    """m3d_fit_multi: one-shot fit from one process driving the devices of `devices`."""
    xyz = _f64(xyz).reshape(-1, 3)
    nrm = _f64(normals).reshape(-1, 3) if normals is not None else None
    n = len(xyz)
    dev = np.ascontiguousarray(devices, dtype=np.int32)
    params = np.zeros(NUM_PARAMS[kind])
    inl = np.empty(max(n, 1), dtype=np.uint64)
    ni = C.c_size_t(0)
    st = Stats()
    _s, sref = _seed_ref(seed)
    rc = _check(lib().m3d_fit_multi(kind, _p(xyz), _p(nrm), n, threshold, max_iteration, probability,
                                    C.cast(sref, C.c_void_p) if sref else None, _p(dev), len(dev), _p(params), _p(inl),
                                    C.cast(C.byref(ni), C.c_void_p), C.cast(C.byref(st), C.c_void_p)))
    d = st.asdict()
    d["n_inliers"] = int(ni.value)
    return Fit(rc, params, inl[: ni.value].copy(), d)


def registration_ransac_sharded(src, dst, corr_src, corr_dst, comm, threshold=0.01, max_iter=100000,
                                edge_length_threshold=0.9, confidence=0.999, seed=None, device=0):
    """m3d_registration_ransac_sharded (every rank of `comm` calls it with the same inputs)."""
    src = _f64(src).reshape(-1, 3)
    dst = _f64(dst).reshape(-1, 3)
    cs = np.ascontiguousarray(corr_src, dtype=np.uint64)
    cd = np.ascontiguousarray(corr_dst, dtype=np.uint64)
    if len(cs) != len(cd):
        raise ValueError("correspondence lists differ in length")
    T = np.zeros(16)
    st = RegStats()
    _s, sref = _seed_ref(seed)
    _check(lib().m3d_registration_ransac_sharded(_p(src), len(src), _p(dst), len(dst), _p(cs), _p(cd), len(cs),
                                                 threshold, max_iter, edge_length_threshold, confidence,
                                                 C.cast(sref, C.c_void_p) if sref else None, device,
                                                 comm._h if comm is not None else None, _p(T),
                                                 C.cast(C.byref(st), C.c_void_p)))
    return T.reshape(4, 4), st.asdict()


def kabsch(src, dst, scaling=False, device=0):
    src = _f64(src).reshape(-1, 3)
    dst = _f64(dst).reshape(-1, 3)
    if len(src) != len(dst):
        raise M3DError(ERR_SIZE_MISMATCH, "The number of points pair is not equal.")
    T = np.zeros(16)
    _check(lib().m3d_kabsch(_p(src), _p(dst), len(src), int(bool(scaling)), device, _p(T)))
    return T.reshape(4, 4)


def kabsch_sums(src, dst, device=0):
    """test hook m3d_bench_kabsch_sums -> the 18 sums m3d_kabsch reads back (6 coordinate sums, 9 covariance sums d s^T,
    3 squared sums of s, the last twelve about the kernels' own means)"""
    src = _f64(src).reshape(-1, 3)
    dst = _f64(dst).reshape(-1, 3)
    if len(src) != len(dst):
        raise M3DError(ERR_SIZE_MISMATCH, "The number of points pair is not equal.")
    out = np.zeros(18)
    _check(lib().m3d_bench_kabsch_sums(_p(src), _p(dst), len(src), device, _p(out)))
    return out


def icp_sums(src, dst, max_correspondence_distance, T, device=0):
    """test hook m3d_bench_icp_sums: one evaluation of the point-to-point ICP step under T -> (out, corr): out[0] = error sum,
    out[1] = count, out[2:20] = the 18 sums of the update, out[20:29] = the moments of the matched target points; corr[i] =
    target index of source point i or -1"""
    src = _f64(src).reshape(-1, 3)
    dst = _f64(dst).reshape(-1, 3)
    Tm = _f64(T).reshape(16).copy()
    out = np.zeros(29)
    corr = np.zeros(max(len(src), 1), dtype=np.int64)
    _check(lib().m3d_bench_icp_sums(_p(src), len(src), _p(dst), len(dst), float(max_correspondence_distance), _p(Tm), device,
                                    _p(out), _p(corr)))
    return out, corr[: len(src)]


def registration_ransac(src, dst, corr_src, corr_dst, threshold=0.01, max_iter=100000, edge_length_threshold=0.9,
                        confidence=0.999, seed=None, device=0):
    src = _f64(src).reshape(-1, 3)
    dst = _f64(dst).reshape(-1, 3)
    cs = np.ascontiguousarray(corr_src, dtype=np.uint64)
    cd = np.ascontiguousarray(corr_dst, dtype=np.uint64)
    if len(cs) != len(cd):
        raise ValueError("correspondence lists differ in length")
    T = np.zeros(16)
    st = RegStats()
    _s, sref = _seed_ref(seed)
    _check(lib().m3d_registration_ransac(_p(src), len(src), _p(dst), len(dst), _p(cs), _p(cd), len(cs), threshold,
                                         max_iter, edge_length_threshold, confidence,
                                         C.cast(sref, C.c_void_p) if sref else None, device, _p(T),
                                         C.cast(C.byref(st), C.c_void_p)))
    return T.reshape(4, 4), st.asdict()


def normals_from_map(xyz, w, h, k=5, view_point=(0.0, 0.0, 0.0), device=0, want_ms=False):
    """m3d_normals_from_map: EstimateNormalsFromMap on an organised point map (h*w, 3) -> (h*w, 3) normals."""
    xyz = _f64(xyz).reshape(-1, 3)
    if len(xyz) != w * h:
        raise M3DError(ERR_INVALID_ARG, "The point cloud size is not equal to given point map size.")
    vp = _f64(view_point).reshape(3).copy()
    out = np.empty((w * h, 3))
    ms = C.c_double(0)
    _check(lib().m3d_normals_from_map(_p(xyz), w, h, k, _p(vp), device, _p(out), C.cast(C.byref(ms), C.c_void_p)))
    return (out, ms.value) if want_ms else out


class IcpStats(C.Structure):
    _fields_ = [("fitness", C.c_double), ("inlier_rmse", C.c_double), ("correspondences", C.c_uint64),
                ("iterations", C.c_int32), ("converged", C.c_int32), ("ms_total", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def registration_icp(src, dst, max_correspondence_distance, init=None, max_iteration=30, relative_fitness=1e-6,
                     relative_rmse=1e-6, device=0, want_correspondences=False):
    """open3d.pipelines.registration.registration_icp(source, target, max_correspondence_distance, init,
    TransformationEstimationPointToPoint(), ICPConvergenceCriteria(...)) -> (T, stats[, correspondences])."""
    src = _f64(src).reshape(-1, 3)
    dst = _f64(dst).reshape(-1, 3)
    Ti = _f64(init).reshape(16).copy() if init is not None else None
    T = np.zeros(16)
    st = IcpStats()
    corr = np.zeros(max(len(src), 1), dtype=np.int64) if want_correspondences else None
    _check(lib().m3d_registration_icp(_p(src), len(src), _p(dst), len(dst), max_correspondence_distance, _p(Ti),
                                      max_iteration, relative_fitness, relative_rmse, device, _p(T),
                                      C.cast(C.byref(st), C.c_void_p), _p(corr)))
    if want_correspondences:
        return T.reshape(4, 4), st.asdict(), corr[: len(src)]
    return T.reshape(4, 4), st.asdict()


def registration_icp_plane(src, dst, dst_normals, max_correspondence_distance, init=None, max_iteration=30,
                           relative_fitness=1e-6, relative_rmse=1e-6, device=0, want_correspondences=False, l1=False):
    """m3d_registration_icp_plane: registration_icp with TransformationEstimationPointToPlane() and the target's normals
    (None: the library's error) -> (T, stats[, correspondences]).  l1=True: m3d_registration_icp_plane_l1, the same call
    with TransformationEstimationPointToPlane(L1Loss())."""
    src = _f64(src).reshape(-1, 3)
    dst = _f64(dst).reshape(-1, 3)
    nrm = _f64(dst_normals).reshape(-1, 3) if dst_normals is not None else None
    if nrm is not None and len(nrm) != len(dst):
        raise ValueError("dst_normals must have one row per target point")
    Ti = _f64(init).reshape(16).copy() if init is not None else None
    T = np.zeros(16)
    st = IcpStats()
    corr = np.zeros(max(len(src), 1), dtype=np.int64) if want_correspondences else None
    call = lib().m3d_registration_icp_plane_l1 if l1 else lib().m3d_registration_icp_plane
    _check(call(_p(src), len(src), _p(dst), _p(nrm), len(dst), max_correspondence_distance, _p(Ti), max_iteration,
                relative_fitness, relative_rmse, device, _p(T), C.cast(C.byref(st), C.c_void_p), _p(corr)))
    if want_correspondences:
        return T.reshape(4, 4), st.asdict(), corr[: len(src)]
    return T.reshape(4, 4), st.asdict()


def _rows(a, like, what):
    """an optional n x 3 array with one row per row of `like`"""
    if a is None:
        return None
    a = _f64(a).reshape(-1, 3)
    if len(a) != len(like):
        raise ValueError(what + " must have one row per point")
    return a


def color_gradient(dst, dst_normals, dst_colors, radius, max_nn=30, device=0):
    """m3d_color_gradient: the per-point colour gradients of coloured ICP (InitializePointCloudForColoredICP) over the Hybrid
    (radius, max_nn) neighbourhoods -> (n, 3)."""
    dst = _f64(dst).reshape(-1, 3)
    nrm, col = _rows(dst_normals, dst, "dst_normals"), _rows(dst_colors, dst, "dst_colors")
    out = np.zeros((max(len(dst), 1), 3))
    _check(lib().m3d_color_gradient(_p(dst), _p(nrm), _p(col), len(dst), float(radius), int(max_nn), device, _p(out)))
    return out[: len(dst)]


def registration_icp_colored(src, src_colors, dst, dst_normals, dst_colors, max_correspondence_distance, init=None,
                             lambda_geometric=0.968, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, device=0,
                             want_correspondences=False):
    """m3d_registration_icp_colored: registration_colored_icp(source, target, max_correspondence_distance, init,
    TransformationEstimationForColoredICP(lambda_geometric), ICPConvergenceCriteria(...)) -> (T, stats[, correspondences]).
    Missing normals or colours (None): the library's error."""
    src = _f64(src).reshape(-1, 3)
    dst = _f64(dst).reshape(-1, 3)
    sc = _rows(src_colors, src, "src_colors")
    nrm, dc = _rows(dst_normals, dst, "dst_normals"), _rows(dst_colors, dst, "dst_colors")
    Ti = _f64(init).reshape(16).copy() if init is not None else None
    T = np.zeros(16)
    st = IcpStats()
    corr = np.zeros(max(len(src), 1), dtype=np.int64) if want_correspondences else None
    _check(lib().m3d_registration_icp_colored(_p(src), _p(sc), len(src), _p(dst), _p(nrm), _p(dc), len(dst),
                                              max_correspondence_distance, lambda_geometric, _p(Ti), max_iteration,
                                              relative_fitness, relative_rmse, device, _p(T), C.cast(C.byref(st), C.c_void_p),
                                              _p(corr)))
    if want_correspondences:
        return T.reshape(4, 4), st.asdict(), corr[: len(src)]
    return T.reshape(4, 4), st.asdict()


REFINE_POINT2POINT_ICP, REFINE_POINT2PLANE_ICP, REFINE_COLORED_ICP, REFINE_GENERALIZED_ICP = 0, 1, 2, 3


class MultiScaleIcpLevel(C.Structure):
    """m3d_multi_scale_icp_level"""
    _fields_ = [("n_src", C.c_uint64), ("n_dst", C.c_uint64), ("icp", IcpStats), ("ms_down_sample", C.c_double),
                ("ms_icp", C.c_double), ("ms_information", C.c_double)]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "icp"}
        d["icp"] = self.icp.asdict()
        return d


def multi_scale_icp(src, dst, voxel_sizes, max_iters, max_correspondence_distance, init=None,
                    method=REFINE_POINT2PLANE_ICP, dst_normals=None, src_normals=None, device=0):
    """m3d_multi_scale_icp: ReconstructionPipeline::MultiScaleICP -> (T (4, 4), information (6, 6), [per-level stats])."""
    src = _f64(src).reshape(-1, 3)
    dst = _f64(dst).reshape(-1, 3)
    dn = _f64(dst_normals).reshape(-1, 3) if dst_normals is not None else None
    sn = _f64(src_normals).reshape(-1, 3) if src_normals is not None else None
    if (dn is not None and len(dn) != len(dst)) or (sn is not None and len(sn) != len(src)):
        raise ValueError("normals must have one row per point")
    sizes = np.ascontiguousarray(voxel_sizes, dtype=np.float64).reshape(-1)
    iters = np.ascontiguousarray(max_iters, dtype=np.int32).reshape(-1)
    if len(sizes) != len(iters):
        raise ValueError("voxel_sizes and max_iters differ in length")
    L = len(sizes)
    Ti = _f64(init).reshape(16).copy() if init is not None else None
    T = np.zeros(16)
    info = np.zeros(36)
    lv = (MultiScaleIcpLevel * max(L, 1))()
    _check(lib().m3d_multi_scale_icp(_p(src), _p(sn), len(src), _p(dst), _p(dn), len(dst), _p(sizes) if L else None,
                                     _p(iters) if L else None, L, float(max_correspondence_distance), int(method), _p(Ti),
                                     device, _p(T), _p(info), C.cast(lv, C.c_void_p)))
    return T.reshape(4, 4), info.reshape(6, 6), [lv[l].asdict() for l in range(L)]


def multi_scale_icp_colored(src, src_colors, dst, dst_normals, dst_colors, voxel_sizes, max_iters, max_correspondence_distance,
                            init=None, lambda_geometric=0.968, src_normals=None, device=0):
    """m3d_multi_scale_icp_colored: MultiScaleICP with LocalRefineMethod::ColoredICP -> (T (4, 4), information (6, 6),
    [per-level stats])."""
    src = _f64(src).reshape(-1, 3)
    dst = _f64(dst).reshape(-1, 3)
    sc, sn = _rows(src_colors, src, "src_colors"), _rows(src_normals, src, "src_normals")
    dn, dc = _rows(dst_normals, dst, "dst_normals"), _rows(dst_colors, dst, "dst_colors")
    sizes = np.ascontiguousarray(voxel_sizes, dtype=np.float64).reshape(-1)
    iters = np.ascontiguousarray(max_iters, dtype=np.int32).reshape(-1)
    if len(sizes) != len(iters):
        raise ValueError("voxel_sizes and max_iters differ in length")
    L = len(sizes)
    Ti = _f64(init).reshape(16).copy() if init is not None else None
    T = np.zeros(16)
    info = np.zeros(36)
    lv = (MultiScaleIcpLevel * max(L, 1))()
    _check(lib().m3d_multi_scale_icp_colored(_p(src), _p(sn), _p(sc), len(src), _p(dst), _p(dn), _p(dc), len(dst),
                                             _p(sizes) if L else None, _p(iters) if L else None, L,
                                             float(max_correspondence_distance), float(lambda_geometric), _p(Ti), device, _p(T),
                                             _p(info), C.cast(lv, C.c_void_p)))
    return T.reshape(4, 4), info.reshape(6, 6), [lv[l].asdict() for l in range(L)]


SEARCH_KNN, SEARCH_RADIUS, SEARCH_HYBRID = 0, 1, 2


def detect_boundary_points(xyz, normals=None, search=SEARCH_HYBRID, radius=0.01, max_nn=30, angle_threshold=90.0,
                           device=0):
    """m3d_detect_boundary_points -> ascending indices (uint64) of the boundary points."""
    xyz = _f64(xyz).reshape(-1, 3)
    nrm = _f64(normals).reshape(-1, 3) if normals is not None else None
    if nrm is not None and len(nrm) != len(xyz):
        raise ValueError("normals and points differ in length")
    out = np.zeros(max(len(xyz), 1), dtype=np.uint64)
    k = C.c_size_t(0)
    _check(lib().m3d_detect_boundary_points(_p(xyz), _p(nrm), len(xyz), search, radius, max_nn, angle_threshold, device,
                                            _p(out), C.cast(C.byref(k), C.c_void_p)))
    return out[: k.value].copy()


FPS_PATH_SINGLE, FPS_PATH_PRUNED, FPS_PATH_DENSE = 1, 2, 3


class FpsStats(C.Structure):
    """m3d_fps_stats"""
    _fields_ = [("ms_total", C.c_double), ("ms_device", C.c_double), ("path", C.c_int32), ("pad", C.c_int32),
                ("tiles_updated", C.c_uint64), ("tile_steps", C.c_uint64)]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}
        d["pruned_fraction"] = 1.0 - self.tiles_updated / self.tile_steps if self.tile_steps else 0.0
        return d


def farthest_point_sampling(xyz, num_samples, device=0, stats=False):
    """m3d_farthest_point_sampling -> the sampled indices (uint64), and the stats dict when stats=True."""
    xyz = _f64(xyz).reshape(-1, 3)
    num_samples = int(num_samples)
    out = np.zeros(max(num_samples, 1), dtype=np.uint64)
    st = FpsStats()
    _check(lib().m3d_farthest_point_sampling(_p(xyz), len(xyz), num_samples, device, _p(out), C.cast(C.byref(st), C.c_void_p)))
    idx = out[: max(num_samples, 0)].copy()
    return (idx, st.asdict()) if stats else idx


def crop_roi_indices(n, roi, shape):
    """m3d_crop_roi_indices: roi = (tl_x, tl_y, br_x, br_y), shape = (width, height) -> the source index of every
    point of CropROIPointCloud's output (uint64)."""
    tl_x, tl_y, br_x, br_y = (int(v) for v in roi)
    width, height = (int(v) for v in shape)
    k = C.c_size_t(0)
    _check(lib().m3d_crop_roi_indices(int(n), width, height, tl_x, tl_y, br_x, br_y, None, C.cast(C.byref(k), C.c_void_p)))
    out = np.zeros(max(k.value, 1), dtype=np.uint64)
    _check(lib().m3d_crop_roi_indices(int(n), width, height, tl_x, tl_y, br_x, br_y, _p(out), C.cast(C.byref(k), C.c_void_p)))
    return out[: k.value].copy()


def fps_force_path(path: int):
    """measurement / test hook m3d_bench_fps_force_path: 0 = by size, FPS_PATH_SINGLE / _PRUNED / _DENSE"""
    _check(lib().m3d_bench_fps_force_path(int(path)))


VOXEL_PATH_PACKED, VOXEL_PATH_WIDE = 1, 2


class VoxelStats(C.Structure):
    """m3d_voxel_stats"""
    _fields_ = [("ms_total", C.c_double), ("ms_upload", C.c_double), ("ms_device", C.c_double), ("ms_download", C.c_double),
                ("n_voxels", C.c_uint64), ("path", C.c_int32), ("sort_passes", C.c_int32)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def _voxel_inputs(xyz, normals, colors):
    xyz = _f64(xyz).reshape(-1, 3)
    normals = _f64(normals).reshape(-1, 3) if normals is not None else None
    colors = _f64(colors).reshape(-1, 3) if colors is not None else None
    for a in (normals, colors):
        if a is not None and len(a) != len(xyz):
            raise ValueError("normals / colors must have one row per point")
    return xyz, normals, colors


def _ptr_array(arrays):
    """a C array of the arrays' addresses (double *const *, size_t *const *), or None when every entry is None"""
    if all(a is None for a in arrays):
        return None
    return (C.c_void_p * len(arrays))(*[_addr(a) for a in arrays])


def voxel_down_sample_multi(xyz, voxel_sizes, normals=None, colors=None, device=0, trace=False, stats=False):
    """m3d_voxel_down_sample_multi: every level from the original cloud -> a list of dicts (points, normals, colors, and
    with trace=True first_index, point_to_voxel as uint64), and the stats dict when stats=True."""
    xyz, normals, colors = _voxel_inputs(xyz, normals, colors)
    sizes = np.ascontiguousarray(voxel_sizes, dtype=np.float64).reshape(-1)
    n, L = len(xyz), len(sizes)
    cap = max(n, 1)
    o_xyz = [np.empty((cap, 3)) for _ in range(L)]
    o_nrm = [np.empty((cap, 3)) if normals is not None else None for _ in range(L)]
    o_col = [np.empty((cap, 3)) if colors is not None else None for _ in range(L)]
    o_first = [np.zeros(cap, dtype=np.uint64) if trace else None for _ in range(L)]
    o_p2v = [np.zeros(cap, dtype=np.uint64) if trace else None for _ in range(L)]
    m = np.zeros(max(L, 1), dtype=np.uint64)
    st = VoxelStats()
    _check(lib().m3d_voxel_down_sample_multi(_p(xyz), _p(normals), _p(colors), n, _p(sizes), L, device, _ptr_array(o_xyz),
                                             _ptr_array(o_nrm), _ptr_array(o_col), _ptr_array(o_first), _ptr_array(o_p2v),
                                             _p(m), C.cast(C.byref(st), C.c_void_p)))
    levels = []
    for l in range(L):
        k = int(m[l])
        d = {"points": o_xyz[l][:k].copy(), "normals": o_nrm[l][:k].copy() if normals is not None else None,
             "colors": o_col[l][:k].copy() if colors is not None else None}
        if trace:
            d["first_index"] = o_first[l][:k].copy()
            d["point_to_voxel"] = o_p2v[l][:n].copy()
        levels.append(d)
    return (levels, st.asdict()) if stats else levels


def voxel_down_sample(xyz, voxel_size, normals=None, colors=None, device=0, trace=False, stats=False):
    """m3d_voxel_down_sample -> dict(points, normals, colors[, first_index, point_to_voxel]): the per-voxel means in
    ascending order of the voxels' lowest member index, and the stats dict when stats=True."""
    xyz, normals, colors = _voxel_inputs(xyz, normals, colors)
    n = len(xyz)
    cap = max(n, 1)
    o_xyz = np.empty((cap, 3))
    o_nrm = np.empty((cap, 3)) if normals is not None else None
    o_col = np.empty((cap, 3)) if colors is not None else None
    o_first = np.zeros(cap, dtype=np.uint64) if trace else None
    o_p2v = np.zeros(cap, dtype=np.uint64) if trace else None
    m = C.c_size_t(0)
    st = VoxelStats()
    _check(lib().m3d_voxel_down_sample(_p(xyz), _p(normals), _p(colors), n, float(voxel_size), device, _p(o_xyz), _p(o_nrm),
                                       _p(o_col), _p(o_first), _p(o_p2v), C.cast(C.byref(m), C.c_void_p),
                                       C.cast(C.byref(st), C.c_void_p)))
    k = m.value
    d = {"points": o_xyz[:k].copy(), "normals": o_nrm[:k].copy() if normals is not None else None,
         "colors": o_col[:k].copy() if colors is not None else None}
    if trace:
        d["first_index"] = o_first[:k].copy()
        d["point_to_voxel"] = o_p2v[:n].copy()
    return (d, st.asdict()) if stats else d


class RaycastMesh(C.Structure):
    """m3d_raycast_mesh"""
    _fields_ = [("vertices", C.c_void_p), ("n_vertices", C.c_size_t), ("triangles", C.c_void_p), ("n_triangles", C.c_size_t)]


class RaycastStats(C.Structure):
    """m3d_raycast_stats"""
    _fields_ = [("ms_total", C.c_double), ("ms_upload", C.c_double), ("ms_build", C.c_double), ("ms_traverse", C.c_double),
                ("ms_download", C.c_double), ("n_triangles", C.c_uint64), ("n_nodes", C.c_uint64), ("n_rays", C.c_uint64),
                ("pair_tests", C.c_uint64), ("nodes_visited", C.c_uint64)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def raycast_pinhole(meshes, pose_lists, camera, device=0, stats=False, outputs=("t_hit", "geometry_ids", "primitive_ids", "normals")):
    """m3d_raycast_pinhole.  meshes: a list of (vertices (n, 3), triangles (m, 3)); pose_lists: F lists of one 4 x 4 pose per
    mesh; camera: (W, H, fx, fy, cx, cy).  -> None when the list of meshes is empty (the call's M3D_FALSE), else a dict of
    the asked-for maps, (F, H, W) each ((F, H, W, 3) the normals), and the stats dict when stats=True."""
    W, H, fx, fy, cx, cy = camera
    W, H = int(W), int(H)
    keep = [(np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(f, dtype=np.int32).reshape(-1, 3))
            for v, f in meshes]
    arr = (RaycastMesh * max(len(keep), 1))()
    for k, (v, f) in enumerate(keep):
        arr[k] = RaycastMesh(v.ctypes.data, len(v), f.ctypes.data, len(f))
    frames = [[np.asarray(T, dtype=np.float64).reshape(4, 4) for T in pl] for pl in pose_lists]
    n_poses = len(frames[0]) if frames else len(keep)
    if any(len(fr) != n_poses for fr in frames):
        raise ValueError("every frame needs the same number of poses")
    poses = np.ascontiguousarray(np.array(frames, dtype=np.float64).reshape(len(frames), n_poses, 4, 4))
    F = len(frames)
    shape = (F, max(H, 0), max(W, 0))
    out = {"t_hit": np.empty(shape, np.float32) if "t_hit" in outputs else None,
           "geometry_ids": np.empty(shape, np.uint32) if "geometry_ids" in outputs else None,
           "primitive_ids": np.empty(shape, np.uint32) if "primitive_ids" in outputs else None,
           "normals": np.empty(shape + (3,), np.float32) if "normals" in outputs else None}
    st = RaycastStats()
    rc = _check(lib().m3d_raycast_pinhole(C.cast(arr, C.c_void_p), len(keep), _p(poses) if poses.size else None, n_poses, F, W, H,
                                          float(fx), float(fy), float(cx), float(cy), device, _p(out["t_hit"]),
                                          _p(out["geometry_ids"]), _p(out["primitive_ids"]), _p(out["normals"]),
                                          C.cast(C.byref(st), C.c_void_p)))
    if rc == FALSE:
        return (None, st.asdict()) if stats else None
    res = {k: v for k, v in out.items() if v is not None}
    return (res, st.asdict()) if stats else res


def voxel_force_path(path: int):
    """measurement / test hook m3d_bench_voxel_force_path: 0 = by the key widths, VOXEL_PATH_PACKED / _WIDE"""
    _check(lib().m3d_bench_voxel_force_path(int(path)))


PROX_DISTANCE, PROX_NORMALS, PROX_DISTANCE_NORMALS = 1, 2, 3
_PROX_KINDS = {"distance": 1, "normals": 2, "distance_normals": 3}
SIZE_MAX = 2**64 - 1


class ProximityEvaluator(C.Structure):
    """m3d_proximity_evaluator"""
    _fields_ = [("kind", C.c_int32), ("pad", C.c_int32), ("dist", C.c_double), ("angle_deg", C.c_double)]


class ProximityStats(C.Structure):
    """m3d_proximity_stats"""
    _fields_ = [("ms_total", C.c_double), ("ms_device", C.c_double), ("ms_order", C.c_double), ("cell_edge", C.c_double),
                ("components", C.c_uint64)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def _prox_call(fn, xyz, normals, kind, dist, angle_deg, min_size, max_size, device, stats, between):
    xyz = _f64(xyz).reshape(-1, 3)
    nrm = None if normals is None else _f64(normals).reshape(-1, 3)
    n = len(xyz)
    ev = ProximityEvaluator(_PROX_KINDS.get(kind, kind), 0, float(dist), float(angle_deg))
    off = np.zeros(n + 1, dtype=np.uint64)
    idx = np.zeros(max(n, 1), dtype=np.uint64)
    lab = np.zeros(max(n, 1), dtype=np.uint64)
    k = C.c_size_t(0)
    st = ProximityStats()
    _check(fn(_p(xyz), _p(nrm), 0 if nrm is None else len(nrm), n, *between(n), C.byref(ev), int(min_size), int(max_size),
              device, _p(off), _p(idx), C.cast(C.byref(k), C.c_void_p), _p(lab), C.cast(C.byref(st), C.c_void_p)))
    off = off[: k.value + 1].copy()
    res = (off, idx[: int(off[-1])].copy(), lab[:n].copy())
    return res + (st.asdict(),) if stats else res


def proximity_segment(xyz, radius, kind, dist=0.0, angle_deg=0.0, normals=None, min_size=1, max_size=SIZE_MAX, device=0,
                      stats=False):
    """m3d_proximity_segment -> (cluster offsets, cluster indices, labels) as uint64 arrays (+ the stats dict)."""
    return _prox_call(lib().m3d_proximity_segment, xyz, normals, kind, dist, angle_deg, min_size, max_size, device, stats,
                      lambda n: (float(radius),))


def proximity_segment_nn(xyz, nn_offsets, nn_indices, kind, dist=0.0, angle_deg=0.0, normals=None, min_size=1,
                         max_size=SIZE_MAX, device=0, stats=False, n_lists=None):
    """m3d_proximity_segment_nn over CSR lists (nn_offsets: n_lists + 1 entries)."""
    off = np.ascontiguousarray(nn_offsets, dtype=np.uint64)
    ind = np.ascontiguousarray(nn_indices, dtype=np.uint64)
    nl = len(off) - 1 if n_lists is None else n_lists
    return _prox_call(lib().m3d_proximity_segment_nn, xyz, normals, kind, dist, angle_deg, min_size, max_size, device, stats,
                      lambda n: (nl, _p(off), _p(ind) if len(ind) else None))


def radius_neighbors(xyz, radius, device=0):
    """m3d_radius_neighbors -> (offsets uint64 (n + 1), indices uint32, d2 float64), each list sorted by (d2, index)"""
    xyz = _f64(xyz).reshape(-1, 3)
    n = len(xyz)
    off = np.zeros(n + 1, dtype=np.uint64)
    tot = C.c_size_t(0)
    _check(lib().m3d_radius_neighbors(_p(xyz), n, float(radius), device, _p(off), None, None, 0,
                                      C.cast(C.byref(tot), C.c_void_p)))
    idx = np.zeros(max(tot.value, 1), dtype=np.uint32)
    d2 = np.zeros(max(tot.value, 1), dtype=np.float64)
    _check(lib().m3d_radius_neighbors(_p(xyz), n, float(radius), device, _p(off), _p(idx), _p(d2), tot.value,
                                      C.cast(C.byref(tot), C.c_void_p)))
    return off, idx[: tot.value].copy(), d2[: tot.value].copy()


KNN_SEARCH_KNN, KNN_SEARCH_HYBRID = 0, 2
KNN_PATH_GRID, KNN_PATH_TILE, KNN_PATH_SELECT = 1, 2, 3


class KnnStats(C.Structure):
    """m3d_knn_stats"""
    _fields_ = [("ms_total", C.c_double), ("ms_device", C.c_double), ("path", C.c_int32), ("launches", C.c_int32),
                ("pair_dims", C.c_uint64), ("tile_queries", C.c_uint64)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class KnnIndex:
    """m3d_knn_create / _search / _destroy: data is N rows of dim doubles (an (N, dim) array = Eigen's dim x N)."""

    def __init__(self, rows, device=0):
        rows = _f64(rows)
        if rows.ndim != 2:
            raise ValueError("rows: expected an (N, dim) array")
        status = C.c_int(0)
        self.h = lib().m3d_knn_create(_p(rows), rows.shape[0], rows.shape[1], device, C.cast(C.byref(status), C.c_void_p))
        if not self.h:
            raise M3DError(status.value, last_error())
        self.n, self.dim = rows.shape

    def close(self):
        if self.h:
            lib().m3d_knn_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def search(self, queries, knn, search=KNN_SEARCH_KNN, radius=0.0, stride=None, want_d2=True, stats=False):
        """-> (indices int64 (m, stride), dist, d2, counts int64 (m,)) (+ the stats dict); padding: -1 / +inf"""
        q = _f64(queries).reshape(-1, self.dim)
        m = len(q)
        kout = min(int(knn), self.n) if knn >= 0 else 0
        stride = kout if stride is None else int(stride)
        idx = np.zeros((m, stride), dtype=np.int64)
        dist = np.zeros((m, stride))
        d2 = np.zeros((m, stride)) if want_d2 else None
        counts = np.zeros(m, dtype=np.int64)
        st = KnnStats()
        _check(lib().m3d_knn_search(self.h, _p(q), m, int(search), int(knn), float(radius), stride, _p(idx), _p(dist),
                                    _p(d2), _p(counts), C.cast(C.byref(st), C.c_void_p)))
        res = (idx, dist, d2, counts)
        return res + (st.asdict(),) if stats else res


def knn_create_status(data_ptr, n, dim, device=0):
    """m3d_knn_create on a raw pointer (argument checks) -> (status code, last error text); the index is destroyed again"""
    status = C.c_int(0)
    h = lib().m3d_knn_create(data_ptr, int(n), int(dim), int(device), C.cast(C.byref(status), C.c_void_p))
    if h:
        lib().m3d_knn_destroy(h)
    return status.value, ("" if h else last_error())


def knn_force_path(path: int):
    """test / measurement hook m3d_bench_knn_force_path: 0 = by shape, KNN_PATH_GRID / TILE / SELECT"""
    _check(lib().m3d_bench_knn_force_path(int(path)))


def knn_tile_merge(data, queries, kk, pages, splits, rows_per_split, device=0):
    """test hook m3d_bench_knn_tile_merge: one chunk of the tile path with the caller's geometry -> (indices uint32, key bits
    uint64), each (m, pages kk), raw: a slot no row fills holds the sentinel (0xFFFFFFFF, all ones)"""
    data = _f64(data)
    if data.ndim != 2:
        raise ValueError("data: expected an (N, dim) array")
    n, dim = data.shape
    q = _f64(queries).reshape(-1, max(dim, 1))
    m = len(q)
    width = max(int(pages), 0) * max(int(kk), 0)
    idx = np.zeros((m, width), dtype=np.uint32)
    key = np.zeros((m, width), dtype=np.uint64)
    _check(lib().m3d_bench_knn_tile_merge(_p(data), n, dim, _p(q), m, int(kk), int(pages), int(splits), int(rows_per_split),
                                          device, _p(idx), _p(key)))
    return idx, key


PPF_PATH_LDS, PPF_PATH_DEVICE = 1, 2


class PpfParams(C.Structure):
    """m3d_ppf_params (angles in radians)"""
    _fields_ = [("rel_sample_dist", C.c_double), ("angle_step", C.c_double), ("min_dist_thresh", C.c_double),
                ("min_angle_thresh", C.c_double), ("faster_mode", C.c_int32), ("reserved", C.c_int32)]


class PpfTableInfo(C.Structure):
    """m3d_ppf_table_info"""
    _fields_ = [("table_size", C.c_uint64), ("n_entries", C.c_uint64), ("n_neighbors", C.c_uint64), ("angle_num", C.c_int32),
                ("alpha_model_num", C.c_int32), ("dist_num", C.c_int32), ("path", C.c_int32)]


class PpfVoteStats(C.Structure):
    """m3d_ppf_vote_stats"""
    _fields_ = [("path", C.c_int32), ("launches", C.c_uint32), ("groups", C.c_uint32), ("reserved", C.c_uint32),
                ("neighbours_visited", C.c_uint64), ("increments", C.c_uint64), ("ms_device", C.c_double), ("ms_total", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


def ppf_params(**kw):
    """the defaults of m3d_ppf_default_params with the given fields replaced"""
    P = PpfParams()
    lib().m3d_ppf_default_params(C.cast(C.byref(P), C.c_void_p))
    for k, v in kw.items():
        if k not in dict(PpfParams._fields_) or k == "reserved":
            raise TypeError(f"ppf_params: no parameter {k!r}")
        setattr(P, k, int(bool(v)) if k == "faster_mode" else float(v))
    return P


def _edge_arrays(edge_points, edge_normals):
    """the scene's (or model's) edge points as two (k, 3) float64 arrays, or (None, None)"""
    if (edge_points is None) != (edge_normals is None):
        raise ValueError("ppf: edge_points and edge_normals come together")
    if edge_points is None:
        return None, None
    ep, en = _f64(edge_points).reshape(-1, 3), _f64(edge_normals).reshape(-1, 3)
    if len(ep) != len(en):
        raise ValueError("ppf: one normal per edge point")
    return ep, en


class PpfModel:
    """m3d_ppf_model_create / _create_edges / _table / m3d_ppf_vote / _vote_edges / _destroy: the PPF table of already sampled model
    points with unit normals, and the vote of a scene against it (include/misc3d_amd.h, "PPF voting").  With edge_points /
    edge_normals the model is trained in EdgePoints mode ("PPF voting, EdgePoints mode") and vote() needs the scene's edge points."""

    def __init__(self, points, normals, diameter, r_min, device=0, edge_points=None, edge_normals=None, **params):
        pts, nrm = _f64(points).reshape(-1, 3), _f64(normals).reshape(-1, 3)
        if len(pts) != len(nrm):
            raise ValueError("ppf: one normal per point")
        if (edge_points is None) != (edge_normals is None):
            raise ValueError("ppf: edge_points and edge_normals come together")
        P = ppf_params(**params)
        status = C.c_int(0)
        if edge_points is None:
            self.h = lib().m3d_ppf_model_create(_p(pts), _p(nrm), len(pts), float(diameter), float(r_min), C.cast(C.byref(P), C.c_void_p),
                                                int(device), C.cast(C.byref(status), C.c_void_p))
        else:
            ep, en = _f64(edge_points).reshape(-1, 3), _f64(edge_normals).reshape(-1, 3)
            if len(ep) != len(en):
                raise ValueError("ppf: one normal per edge point")
            self.h = lib().m3d_ppf_model_create_edges(_p(pts), _p(nrm), len(pts), _p(ep), _p(en), len(ep), float(diameter), float(r_min),
                                                      C.cast(C.byref(P), C.c_void_p), int(device), C.cast(C.byref(status), C.c_void_p))
        if not self.h:
            raise M3DError(status.value, last_error())
        self.n = len(pts)
        self.n_edge = int(lib().m3d_ppf_model_edge_size(self.h))
        self.device = int(device)
        c = np.zeros(3)
        _check(lib().m3d_ppf_model_centroid(self.h, _p(c)))
        self.centroid = c

    def close(self):
        if getattr(self, "h", None):
            lib().m3d_ppf_model_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def info(self):
        I = PpfTableInfo()
        _check(lib().m3d_ppf_model_table(self.h, C.cast(C.byref(I), C.c_void_p), None, None, None, None, None, None))
        return {k: int(getattr(I, k)) for k, _ in PpfTableInfo._fields_}

    def table(self):
        """-> dict(cell_offsets, entry_i, entry_alpha, nbr_offsets, nbr_indices, tmg (n, 4, 4), centroid) + the info fields"""
        I = self.info()
        t = dict(cell_offsets=np.zeros(I["table_size"] + 1, np.uint32), entry_i=np.zeros(I["n_entries"], np.uint16),
                 entry_alpha=np.zeros(I["n_entries"], np.uint8), nbr_offsets=np.zeros(self.n + 1, np.uint32),
                 nbr_indices=np.zeros(I["n_neighbors"], np.uint32), tmg=np.zeros((self.n, 4, 4)))
        _check(lib().m3d_ppf_model_table(self.h, None, *(_p(t[k]) for k in ("cell_offsets", "entry_i", "entry_alpha", "nbr_offsets",
                                                                             "nbr_indices", "tmg"))))
        t["centroid"] = self.centroid.copy()
        t.update(I)
        return t

    def vote(self, scene_points, scene_normals, reference, capacity=None, stats=False, edge_points=None, edge_normals=None):
        """-> dict(ref_pos, model_index, alpha_index, votes (uint32 each), poses (K, 4, 4)) (+ the stats dict).  capacity=None:
        the call is repeated once with the needed capacity when the first guess was too small; a given capacity is final
        (M3DError with code ERR_CAPACITY and .needed set).  edge_points / edge_normals: the scene's edge points, which send the
        call through m3d_ppf_vote_edges (the library refuses the call that does not match the model's mode)."""
        sp, sn = _f64(scene_points).reshape(-1, 3), _f64(scene_normals).reshape(-1, 3)
        if len(sp) != len(sn):
            raise ValueError("ppf: one normal per scene point")
        ep, en = _edge_arrays(edge_points, edge_normals)
        ref = np.ascontiguousarray(reference, dtype=np.uint64).reshape(-1)
        cap = max(256, 4 * len(ref)) if capacity is None else int(capacity)
        while True:
            out = [np.zeros(max(cap, 1), np.uint32) for _ in range(4)]
            poses = np.zeros((max(cap, 1), 4, 4))
            k = C.c_size_t(0)
            st = PpfVoteStats()
            if ep is None:
                rc = lib().m3d_ppf_vote(self.h, _p(sp), _p(sn), len(sp), _p(ref), len(ref), cap, C.cast(C.byref(k), C.c_void_p),
                                        *(_p(o) for o in out), _p(poses), C.cast(C.byref(st), C.c_void_p))
            else:
                rc = lib().m3d_ppf_vote_edges(self.h, _p(sp), _p(sn), len(sp), _p(ref), len(ref), _p(ep), _p(en), len(ep), cap,
                                              C.cast(C.byref(k), C.c_void_p), *(_p(o) for o in out), _p(poses),
                                              C.cast(C.byref(st), C.c_void_p))
            if rc == ERR_CAPACITY and capacity is None:
                cap = k.value
                continue
            if rc < 0:
                e = M3DError(rc, last_error())
                e.needed = k.value
                raise e
            break
        res = dict(ref_pos=out[0][:k.value], model_index=out[1][:k.value], alpha_index=out[2][:k.value], votes=out[3][:k.value],
                   poses=poses[:k.value])
        return (res, st.asdict()) if stats else res


PPF_REFINE_NONE, PPF_REFINE_POINT_TO_POINT, PPF_REFINE_POINT_TO_PLANE = 0, 1, 2
PPF_REFINE_METHODS = {"NoRefine": PPF_REFINE_NONE, "PointToPoint": PPF_REFINE_POINT_TO_POINT, "PointToPlane": PPF_REFINE_POINT_TO_PLANE}


class PpfClusterParams(C.Structure):
    """m3d_ppf_cluster_params (angle in radians)"""
    _fields_ = [("dist_threshold", C.c_double), ("angle_threshold", C.c_double), ("ratio", C.c_double), ("score_thresh", C.c_double),
                ("rel_dist_sparse_thresh", C.c_double), ("num_result", C.c_int32), ("refine_method", C.c_int32),
                ("object_id", C.c_int32), ("reserved", C.c_int32)]


class PpfClusterStats(C.Structure):
    """m3d_ppf_cluster_stats"""
    _fields_ = [("n_valid", C.c_uint64), ("clusters_t", C.c_uint64), ("clusters_r", C.c_uint64), ("pair_tests", C.c_uint64),
                ("launches", C.c_uint32), ("splits", C.c_uint32), ("ms_device", C.c_double), ("ms_total", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PpfEstimateStats(C.Structure):
    """m3d_ppf_estimate_stats"""
    _fields_ = [("vote", PpfVoteStats), ("cluster", PpfClusterStats), ("n_raw", C.c_uint64), ("icp_calls", C.c_uint32),
                ("icp_iterations", C.c_uint32), ("ms_vote", C.c_double), ("ms_cluster", C.c_double), ("ms_refine", C.c_double),
                ("ms_host", C.c_double), ("ms_total", C.c_double)]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("vote", "cluster")}
        d["vote"], d["cluster"] = self.vote.asdict(), self.cluster.asdict()
        return d


def ppf_cluster_params(model=None, **kw):
    """the defaults of m3d_ppf_default_cluster_params (dist_threshold = 0.05 x the model's diameter; 0.05 without a model) with
    the given fields replaced; refine_method may be one of the reference's names (NoRefine, PointToPoint, PointToPlane)"""
    P = PpfClusterParams()
    lib().m3d_ppf_default_cluster_params(model.h if model is not None else None, C.cast(C.byref(P), C.c_void_p))
    for k, v in kw.items():
        if k not in dict(PpfClusterParams._fields_) or k == "reserved":
            raise TypeError(f"ppf_cluster_params: no parameter {k!r}")
        if k == "refine_method" and isinstance(v, str):
            v = PPF_REFINE_METHODS[v]
        setattr(P, k, int(v) if k in ("num_result", "refine_method", "object_id") else float(v))
    return P


def ppf_cluster_poses(poses, votes, device=0, model=None, pose_capacity=None, cluster_capacity=None, **params):
    """m3d_ppf_cluster_poses (K1 - K6 of "PPF pose clustering") -> dict(order, count_t, label_t, count_r, label_r (per valid pose),
    min_num_pt_t, min_num_pt_r, cluster_votes (per translation cluster), avg_poses (K, 4, 4), avg_votes, avg_cluster, stats).
    Capacities None: the call is repeated once with the needed ones; given capacities are final (M3DError with code
    ERR_CAPACITY and .needed = (n_valid, clusters_t, clusters_r))."""
    T = _f64(poses).reshape(-1, 4, 4)
    v = np.ascontiguousarray(votes, dtype=np.uint32).reshape(-1)
    if len(T) != len(v):
        raise ValueError("ppf: one vote count per pose")
    P = ppf_cluster_params(model, **params)
    fixed = pose_capacity is not None or cluster_capacity is not None
    pcap = len(T) if pose_capacity is None else int(pose_capacity)
    ccap = 64 if cluster_capacity is None else int(cluster_capacity)
    while True:
        per_pose = [np.zeros(max(pcap, 1), dt) for dt in (np.uint32, np.uint32, np.int32, np.uint32, np.int32)]
        min_r, cvotes = np.zeros(max(ccap, 1), np.int32), np.zeros(max(ccap, 1), np.uint64)
        avg, avotes, acl = np.zeros((max(ccap, 1), 4, 4)), np.zeros(max(ccap, 1), np.uint64), np.zeros(max(ccap, 1), np.uint32)
        nv, nt, nr, min_t = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
        st = PpfClusterStats()
        ref = lambda x: C.cast(C.byref(x), C.c_void_p)
        rc = lib().m3d_ppf_cluster_poses(_p(T), _p(v), len(T), ref(P), int(device), pcap, ref(nv), *(_p(a) for a in per_pose), ccap,
                                         ref(nt), ref(nr), ref(min_t), _p(min_r), _p(cvotes), _p(avg), _p(avotes), _p(acl), ref(st))
        if rc == ERR_CAPACITY and not fixed and (nv.value > pcap or max(nt.value, nr.value) > ccap):
            pcap, ccap, fixed = max(pcap, nv.value), max(ccap, nt.value, nr.value), True
            continue
        if rc < 0:
            e = M3DError(rc, last_error())
            e.needed = (nv.value, nt.value, nr.value)
            raise e
        break
    n, ct, cr = nv.value, nt.value, nr.value
    return dict(order=per_pose[0][:n], count_t=per_pose[1][:n], label_t=per_pose[2][:n], count_r=per_pose[3][:n], label_r=per_pose[4][:n],
                min_num_pt_t=int(min_t.value), min_num_pt_r=min_r[:ct], cluster_votes=cvotes[:ct], avg_poses=avg[:cr],
                avg_votes=avotes[:cr], avg_cluster=acl[:cr], stats=st.asdict())


def ppf_estimate(model, scene_points, scene_normals, reference, capacity=None, edge_points=None, edge_normals=None, **params):
    """m3d_ppf_estimate (the vote and K1 - K8) on a PpfModel -> dict(poses (K, 4, 4), q (K, 4), t (K, 3), votes, scores, object_id,
    stats).  edge_points / edge_normals: the scene's edge points, which send the call through m3d_ppf_estimate_edges."""
    sp, sn = _f64(scene_points).reshape(-1, 3), _f64(scene_normals).reshape(-1, 3)
    if len(sp) != len(sn):
        raise ValueError("ppf: one normal per scene point")
    ep, en = _edge_arrays(edge_points, edge_normals)
    ref = np.ascontiguousarray(reference, dtype=np.uint64).reshape(-1)
    P = ppf_cluster_params(model, **params)
    cap = max(int(P.num_result), 1) if capacity is None else int(capacity)
    poses, q, t = np.zeros((max(cap, 1), 4, 4)), np.zeros((max(cap, 1), 4)), np.zeros((max(cap, 1), 3))
    votes, scores = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1))
    k = C.c_size_t(0)
    st = PpfEstimateStats()
    if ep is None:
        rc = lib().m3d_ppf_estimate(model.h, _p(sp), _p(sn), len(sp), _p(ref), len(ref), C.cast(C.byref(P), C.c_void_p), cap,
                                    C.cast(C.byref(k), C.c_void_p), _p(poses), _p(q), _p(t), _p(votes), _p(scores), C.cast(C.byref(st), C.c_void_p))
    else:
        rc = lib().m3d_ppf_estimate_edges(model.h, _p(sp), _p(sn), len(sp), _p(ref), len(ref), _p(ep), _p(en), len(ep),
                                          C.cast(C.byref(P), C.c_void_p), cap, C.cast(C.byref(k), C.c_void_p), _p(poses), _p(q), _p(t),
                                          _p(votes), _p(scores), C.cast(C.byref(st), C.c_void_p))
    if rc < 0:
        e = M3DError(rc, last_error())
        e.needed = k.value
        raise e
    n = k.value
    return dict(poses=poses[:n], q=q[:n], t=t[:n], votes=votes[:n], scores=scores[:n], object_id=int(P.object_id), stats=st.asdict())


def ppf_prepare_scene(points, normals, diameter, calc_normal_relative, dist_step, dist_step_dense=0.0, pts_num=30, device=0):
    """m3d_ppf_prepare_scene (PreprocessEstimate): normals may be None (then estimated); dist_step_dense <= 0: no edge part.
    -> dict(sample_points, sample_normals, dense_points, dense_normals ((k, 3) each), edge_indices (into the dense sample,
    ascending))"""
    xyz = _f64(points).reshape(-1, 3)
    nrm = None if normals is None else _f64(normals).reshape(-1, 3)
    if nrm is not None and len(nrm) != len(xyz):
        raise ValueError("ppf: one normal per point")
    n = len(xyz)
    dense = bool(dist_step_dense > 0.0)
    sp, sn = np.zeros((max(n, 1), 3)), np.zeros((max(n, 1), 3))
    dp, dn = (np.zeros((max(n, 1), 3)), np.zeros((max(n, 1), 3))) if dense else (None, None)
    ei = np.zeros(max(n, 1), np.uint64) if dense else None
    ns, nd, ne = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    ref = lambda x: C.cast(C.byref(x), C.c_void_p)
    _check(lib().m3d_ppf_prepare_scene(_p(xyz), _p(nrm), n, float(diameter), float(calc_normal_relative), float(dist_step),
                                       float(dist_step_dense), int(pts_num), int(device), _p(sp), _p(sn), ref(ns), _p(dp), _p(dn),
                                       ref(nd), _p(ei), ref(ne)))
    return dict(sample_points=sp[:ns.value].copy(), sample_normals=sn[:ns.value].copy(),
                dense_points=dp[:nd.value].copy() if dense else np.zeros((0, 3)),
                dense_normals=dn[:nd.value].copy() if dense else np.zeros((0, 3)),
                edge_indices=ei[:ne.value].astype(np.int64) if dense else np.zeros(0, np.int64))


class OrientStats(C.Structure):
    """m3d_orient_stats"""
    _fields_ = [("rounds", C.c_uint64), ("tree_edges", C.c_uint64), ("component", C.c_uint64), ("flips", C.c_uint64),
                ("ms_total", C.c_double), ("ms_grid", C.c_double), ("ms_rounds", C.c_double), ("ms_signs", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PpfTrainParams(C.Structure):
    """m3d_ppf_train_params"""
    _fields_ = [("rel_sample_dist", C.c_double), ("rel_dense_sample_dist", C.c_double), ("calc_normal_relative", C.c_double),
                ("invert_model_normal", C.c_int32), ("use_external_normal", C.c_int32), ("pts_num", C.c_int32), ("reserved", C.c_int32)]


class PpfModelInfo(C.Structure):
    """m3d_ppf_model_info"""
    _fields_ = [("box_center", C.c_double * 3), ("box_extent", C.c_double * 3), ("diameter", C.c_double), ("r_min", C.c_double),
                ("dist_step", C.c_double), ("dist_step_dense", C.c_double), ("normal_r", C.c_double), ("view_pt", C.c_double * 3),
                ("seed", C.c_uint64), ("seed_flipped", C.c_int32), ("oriented", C.c_int32), ("orient", OrientStats),
                ("sample_distance_evaluations", C.c_uint64), ("dense_distance_evaluations", C.c_uint64), ("ms_total", C.c_double),
                ("ms_box", C.c_double), ("ms_normals", C.c_double), ("ms_sample", C.c_double), ("ms_dense", C.c_double),
                ("ms_edges", C.c_double)]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        for k in ("box_center", "box_extent", "view_pt"):
            d[k] = np.array(d[k][:])
        d["orient"] = self.orient.asdict()
        return d


def orient_normals_mst(points, normals, radius, seed, device=0):
    """m3d_orient_normals_mst (rules O1 - O5) -> (oriented normals (n, 3), parent (n,) int64, the stats dict)"""
    xyz, nrm = _f64(points).reshape(-1, 3), _f64(normals).reshape(-1, 3)
    if len(nrm) != len(xyz):
        raise ValueError("orient normals: one normal per point")
    out, parent = np.zeros((max(len(xyz), 1), 3)), np.zeros(max(len(xyz), 1), np.int64)
    st = OrientStats()
    if int(seed) < 0:
        raise ValueError("orient normals: the seed is an index")
    _check(lib().m3d_orient_normals_mst(_p(xyz), _p(nrm), len(xyz), float(radius), int(seed), int(device), _p(out), _p(parent),
                                        C.cast(C.byref(st), C.c_void_p)))
    return out[:len(xyz)], parent[:len(xyz)], st.asdict()


def ppf_train_params(**kw):
    """m3d_ppf_train_params_default_ with the given fields changed"""
    P = PpfTrainParams()
    lib().m3d_ppf_train_params_default_(C.cast(C.byref(P), C.c_void_p))
    for k, v in kw.items():
        if k not in dict(PpfTrainParams._fields_) or k == "reserved":
            raise TypeError("ppf train params: unknown field " + k)
        setattr(P, k, v)
    return P


def ppf_prepare_model(points, normals=None, box_center=None, box_extent=None, device=0, **params):
    """m3d_ppf_prepare_model (PreprocessTrain, rules B1 - B6): normals may be None (then estimated); params: the fields of
    m3d_ppf_train_params.  -> dict(normals (n, 3), sample_indices, dense_indices, edge_indices (into the dense sample), info)"""
    xyz = _f64(points).reshape(-1, 3)
    nrm = None if normals is None else _f64(normals).reshape(-1, 3)
    if nrm is not None and len(nrm) != len(xyz):
        raise ValueError("ppf: one normal per point")
    if (box_center is None) != (box_extent is None):
        raise ValueError("ppf: box_center and box_extent come together")
    bc = None if box_center is None else _f64(box_center).reshape(3)
    be = None if box_extent is None else _f64(box_extent).reshape(3)
    P = ppf_train_params(**params)
    n = len(xyz)
    out = np.zeros((max(n, 1), 3))
    si, di, ei = (np.zeros(max(n, 1), np.uint64) for _ in range(3))
    ns, nd, ne = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    info = PpfModelInfo()
    ref = lambda x: C.cast(C.byref(x), C.c_void_p)
    _check(lib().m3d_ppf_prepare_model(_p(xyz), _p(nrm), n, ref(P), _p(bc), _p(be), int(device), _p(out), _p(si), ref(ns), _p(di),
                                       ref(nd), _p(ei), ref(ne), ref(info)))
    return dict(normals=out[:n], sample_indices=si[:ns.value].astype(np.int64), dense_indices=di[:nd.value].astype(np.int64),
                edge_indices=ei[:ne.value].astype(np.int64), info=info.asdict())


def ppf_reference_indices(num, sample, seed):
    """m3d_ppf_reference_indices: SampleWithoutDuplicate(sample) of RandomSampler(num) on std::mt19937(seed) -> (sample,) int64"""
    out = np.zeros(max(int(sample), 1), np.uint64)
    _check(lib().m3d_ppf_reference_indices(int(num), int(sample), int(seed) & 0xFFFFFFFF, _p(out)))
    return out[:int(sample)].astype(np.int64)


def ppf_cluster_force(splits=0):
    """test / measurement hook m3d_bench_ppf_cluster_force: `splits` workgroups share the j tiles of a row block (0: default)"""
    _check(lib().m3d_bench_ppf_cluster_force(int(splits)))


def ppf_force(device_memory_path=False, max_groups=0):
    """test / measurement hook m3d_bench_ppf_force: accumulators in device memory, at most max_groups workgroups (0: default)"""
    _check(lib().m3d_bench_ppf_force(int(bool(device_memory_path)), int(max_groups)))


_scratch_pattern = -1   # what m3d_bench_scratch_fill was last set to (the library starts with the hook off)


@contextlib.contextmanager
def scratch_fill(pattern):
    """test hook m3d_bench_scratch_fill: inside the block every piece of scratch the library hands out is set to the byte
    `pattern` (0..255; -1: left as it is) first; the previous setting comes back on exit.  Switching resets scratch_fill_stats."""
    global _scratch_pattern
    prev = _scratch_pattern
    _check(lib().m3d_bench_scratch_fill(int(pattern)))
    _scratch_pattern = int(pattern)
    try:
        yield
    finally:
        _check(lib().m3d_bench_scratch_fill(prev))
        _scratch_pattern = prev


def scratch_fill_stats():
    """m3d_bench_scratch_fill_stats -> (blocks, bytes) filled since the hook was last switched"""
    out = np.zeros(2, np.uint64)
    _check(lib().m3d_bench_scratch_fill_stats(_p(out)))
    return int(out[0]), int(out[1])


def scratch_probe(nbytes, device=0):
    """m3d_bench_scratch_probe -> 128 uint8: the first and the last 64 bytes of a block of device scratch of `nbytes` bytes as handed out"""
    out = np.zeros(128, np.uint8)
    _check(lib().m3d_bench_scratch_probe(int(device), int(nbytes), _p(out)))
    return out


class FpfhStats(C.Structure):
    """m3d_fpfh_stats (= m3d_normals_stats)"""
    _fields_ = [("ms_total", C.c_double), ("ms_device", C.c_double), ("ms_upload", C.c_double), ("ms_search", C.c_double),
                ("ms_normals", C.c_double), ("ms_spfh", C.c_double), ("ms_fpfh", C.c_double), ("pairs", C.c_uint64),
                ("pairs_seen", C.c_uint64), ("launches", C.c_int32), ("searches", C.c_int32), ("tie_points", C.c_uint64)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def estimate_normals(xyz, search=SEARCH_HYBRID, radius=0.1, max_nn=30, orient_to=None, device=0, stats=False):
    """m3d_estimate_normals -> (N, 3) normals (+ the stats dict).  orient_to: a camera location (3 numbers) or None."""
    xyz = _f64(xyz).reshape(-1, 3)
    cam = _f64(orient_to).reshape(3) if orient_to is not None else None
    out = np.zeros((len(xyz), 3))
    st = FpfhStats()
    _check(lib().m3d_estimate_normals(_p(xyz), len(xyz), int(search), float(radius), int(max_nn), int(cam is not None),
                                      _p(cam), device, _p(out), C.cast(C.byref(st), C.c_void_p)))
    return (out, st.asdict()) if stats else out


def compute_fpfh_feature(xyz, normals, search=SEARCH_HYBRID, radius=0.1, max_nn=100, device=0, stats=False):
    """m3d_compute_fpfh -> (N, 33) C-contiguous = Eigen's column-major 33 x N (+ the stats dict)."""
    xyz = _f64(xyz).reshape(-1, 3)
    nrm = _f64(normals).reshape(-1, 3) if normals is not None else None
    if nrm is not None and len(nrm) != len(xyz):
        raise ValueError("normals and points differ in length")
    out = np.zeros((len(xyz), 33))
    st = FpfhStats()
    _check(lib().m3d_compute_fpfh(_p(xyz), _p(nrm), len(xyz), int(search), float(radius), int(max_nn), device, _p(out),
                                  C.cast(C.byref(st), C.c_void_p)))
    return (out, st.asdict()) if stats else out


def preprocess_fragment(xyz, voxel_size, normals=None, device=0, stats=False):
    """m3d_preprocess_fragment -> ((N, 3) normals, (N, 33) descriptors) (+ the stats dict)."""
    xyz = _f64(xyz).reshape(-1, 3)
    nrm = _f64(normals).reshape(-1, 3) if normals is not None else None
    if nrm is not None and len(nrm) != len(xyz):
        raise ValueError("normals and points differ in length")
    out_n = np.zeros((len(xyz), 3))
    out_f = np.zeros((len(xyz), 33))
    st = FpfhStats()
    _check(lib().m3d_preprocess_fragment(_p(xyz), _p(nrm), len(xyz), float(voxel_size), device, _p(out_n), _p(out_f),
                                         C.cast(C.byref(st), C.c_void_p)))
    return (out_n, out_f, st.asdict()) if stats else (out_n, out_f)


def fpfh_pair_bins(pairs, features=False):
    """test hook m3d_bench_fpfh_pair_bins: pairs (m, 12) = (p1, n1, p2, n2) -> bins int32 (m, 3) (+ features (m, 3))"""
    pairs = _f64(pairs).reshape(-1, 12)
    bins = np.zeros((len(pairs), 3), dtype=np.int32)
    f = np.zeros((len(pairs), 3)) if features else None
    _check(lib().m3d_bench_fpfh_pair_bins(_p(pairs), len(pairs), _p(bins), _p(f)))
    return (bins, f) if features else bins


def fpfh_stages(xyz, normals, search=SEARCH_HYBRID, radius=0.1, max_nn=100, device=0):
    """test hook m3d_bench_fpfh_stages -> dict, everything by point index: list_idx uint32 (N, max_nn), list_d2 (N, max_nn), cnt
    uint32 (N,), spfh_count uint8 (N, 33), spfh_incr (N,), tie_points uint32 (n_ties,) ascending, feature (N, 33), stats"""
    xyz = _f64(xyz).reshape(-1, 3)
    nrm = _f64(normals).reshape(-1, 3)
    if len(nrm) != len(xyz):
        raise ValueError("normals and points differ in length")
    n, k = len(xyz), max(int(max_nn), 0)
    o = dict(list_idx=np.zeros((n, k), np.uint32), list_d2=np.zeros((n, k)), cnt=np.zeros(n, np.uint32),
             spfh_count=np.zeros((n, 33), np.uint8), spfh_incr=np.zeros(n), tie_points=np.zeros(n, np.uint32),
             feature=np.zeros((n, 33)))
    nt = C.c_uint64(0)
    st = FpfhStats()
    _check(lib().m3d_bench_fpfh_stages(_p(xyz), _p(nrm), n, int(search), float(radius), int(max_nn), device, _p(o["list_idx"]),
                                       _p(o["list_d2"]), _p(o["cnt"]), _p(o["spfh_count"]), _p(o["spfh_incr"]),
                                       _p(o["tie_points"]), C.cast(C.byref(nt), C.c_void_p), _p(o["feature"]),
                                       C.cast(C.byref(st), C.c_void_p)))
    o["tie_points"] = o["tie_points"][:nt.value].copy()
    o["n_ties"] = int(nt.value)
    o["stats"] = st.asdict()
    return o


def proximity_cutoffs(dist, angle_deg):
    """test hook m3d_bench_proximity_cutoffs -> (d2_cut, lo1, hi1, lo2, hi2)"""
    out = np.zeros(5)
    _check(lib().m3d_bench_proximity_cutoffs(float(dist), float(angle_deg), _p(out)))
    return tuple(float(v) for v in out)


def radius_grid_geom(lo, hi, edge, k0):
    """test hook m3d_bench_radius_grid_geom -> (K, h, (nx, ny, nz)): the rung of the cell-table ladder for the box [lo, hi]"""
    lo = _f64(lo).reshape(3)
    hi = _f64(hi).reshape(3)
    K = C.c_int(0)
    h = C.c_double(0.0)
    dims = np.zeros(3, dtype=np.uint64)
    _check(lib().m3d_bench_radius_grid_geom(_p(lo), _p(hi), float(edge), int(k0), C.cast(C.byref(K), C.c_void_p),
                                            C.cast(C.byref(h), C.c_void_p), _p(dims)))
    return int(K.value), float(h.value), tuple(int(d) for d in dims)


def reg_grid_k0(k_cfg, n_dst):
    """test hook m3d_bench_reg_grid_k0: the K0 of the registration validation's grid for reg_cells_per_radius = k_cfg"""
    return int(lib().m3d_bench_reg_grid_k0(int(k_cfg), int(n_dst)))


def information_matrix(src, dst, max_correspondence_distance, T, device=0):
    """GetInformationMatrixFromPointClouds -> (6 x 6 information matrix, correspondence count)."""
    src = _f64(src).reshape(-1, 3)
    dst = _f64(dst).reshape(-1, 3)
    Tm = _f64(T).reshape(16).copy()
    info = np.zeros(36)
    nc = C.c_uint64(0)
    _check(lib().m3d_information_matrix(_p(src), len(src), _p(dst), len(dst), max_correspondence_distance, _p(Tm),
                                        device, _p(info), C.cast(C.byref(nc), C.c_void_p)))
    return info.reshape(6, 6), int(nc.value)


class GlobalRegStats(C.Structure):
    """m3d_global_reg_stats"""
    _fields_ = [("n_matches", C.c_uint64), ("n_info_correspondences", C.c_uint64), ("identity_shortcut", C.c_int32),
                ("device", C.c_int32), ("lane", C.c_int32), ("reserved_", C.c_int32), ("ms_match", C.c_double),
                ("ms_ransac", C.c_double), ("ms_info", C.c_double), ("ms_total", C.c_double), ("ransac", RegStats)]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("ransac", "reserved_")}
        d["ransac"] = self.ransac.asdict()
        return d


class FragmentPair(C.Structure):
    """m3d_fragment_pair"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("n_src", C.c_size_t), ("n_dst", C.c_size_t),
                ("feat_src", C.c_void_p), ("feat_dst", C.c_void_p), ("seed", C.c_uint64), ("has_seed", C.c_int32),
                ("rc", C.c_int32), ("T", C.c_double * 16), ("info", C.c_double * 36), ("stats", GlobalRegStats)]


def _pair_arrays(src, dst, feat_src, feat_dst):
    src = _f64(src).reshape(-1, 3)
    dst = _f64(dst).reshape(-1, 3)
    fs = _f64(feat_src)
    fd = _f64(feat_dst)
    if fs.ndim != 2 or fd.ndim != 2 or fs.shape[1] != fd.shape[1] or len(fs) != len(src) or len(fd) != len(dst):
        raise ValueError("descriptor matrices must be (N, dim), one row per point, equal dim")
    return src, dst, fs, fd


def global_registration(src, dst, feat_src, feat_dst, voxel_size, max_iter=100000, edge_length_threshold=0.9,
                        confidence=0.999, seed=None, device=0, want_stats=False):
    """m3d_global_registration = ReconstructionPipeline::GlobalRegistration with the Ransac method
    (src/pipeline.cpp:790-828): mutual-NN match -> RANSACSolver(1.4 voxel) -> isIdentity shortcut -> information matrix;
    rejected when info(5,5) / min(Ns, Nt) < 0.3.  Returns (success, pose 4x4, information 6x6[, stats])."""
    src, dst, fs, fd = _pair_arrays(src, dst, feat_src, feat_dst)
    T = np.zeros(16)
    info = np.zeros(36)
    st = GlobalRegStats()
    _s, sref = _seed_ref(seed)
    f = lib().m3d_global_registration
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int,
                  C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = _check(f(_p(src), len(src), _p(dst), len(dst), _p(fs), _p(fd), fs.shape[1], float(voxel_size), int(max_iter),
                  float(edge_length_threshold), float(confidence), C.cast(sref, C.c_void_p) if sref else None, device,
                  _p(T), _p(info), C.cast(C.byref(st), C.c_void_p)))
    out = (rc == 1, T.reshape(4, 4), info.reshape(6, 6))
    return out + (st.asdict(),) if want_stats else out


def global_registration_batch(pairs, voxel_size, max_iter=100000, edge_length_threshold=0.9, confidence=0.999, seeds=None,
                              devices=(0,), inflight=0, want_stats=False):
    """m3d_global_registration_batch: pairs = [(src, dst, feat_src, feat_dst), ...] (BuildPoseGraphForScene's loop over
    fragment pairs, src/pipeline.cpp:428-439) -> [(success, pose, information[, stats]), ...] in the order given.
    seeds: one per pair or None."""
    arrs = [_pair_arrays(*p) for p in pairs]
    n = len(arrs)
    if n == 0:
        return []
    dim = arrs[0][2].shape[1]
    if any(a[2].shape[1] != dim for a in arrs):
        raise ValueError("every pair must use descriptors of the same width")
    fp = (FragmentPair * n)()
    for k, (src, dst, fs, fd) in enumerate(arrs):
        fp[k].src, fp[k].dst, fp[k].n_src, fp[k].n_dst = _addr(src), _addr(dst), len(src), len(dst)
        fp[k].feat_src, fp[k].feat_dst = _addr(fs), _addr(fd)
        if seeds is not None and seeds[k] is not None:
            fp[k].seed, fp[k].has_seed = int(seeds[k]) & 0xFFFFFFFFFFFFFFFF, 1
    dev = (C.c_int * len(devices))(*[int(d) for d in devices])
    f = lib().m3d_global_registration_batch
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_int]
    _check(f(C.cast(fp, C.c_void_p), n, dim, float(voxel_size), int(max_iter), float(edge_length_threshold),
             float(confidence), C.cast(dev, C.c_void_p), len(devices), int(inflight)))
    out = []
    for k in range(n):
        r = (fp[k].rc == 1, np.array(fp[k].T).reshape(4, 4), np.array(fp[k].info).reshape(6, 6))
        out.append(r + (fp[k].stats.asdict(),) if want_stats else r)
    return out


class FragmentView(C.Structure):
    """m3d_fragment_view"""
    _fields_ = [("xyz", C.c_void_p), ("feat", C.c_void_p), ("n", C.c_size_t)]


class PairResult(C.Structure):
    """m3d_pair_result"""
    _fields_ = [("s", C.c_int32), ("t", C.c_int32), ("has_seed", C.c_int32), ("rc", C.c_int32), ("seed", C.c_uint64),
                ("T", C.c_double * 16), ("info", C.c_double * 36), ("stats", GlobalRegStats)]


def register_fragment_pairs(fragments, features, pairs, voxel_size, max_iter=100000, edge_length_threshold=0.9,
                            confidence=0.999, seeds=None, devices=(0,), inflight=0, want_stats=False):
    """m3d_register_fragment_pairs: fragments[i] (N_i, 3), features[i] (N_i, dim), pairs = [(s, t), ...] -> [(success, pose,
    information[, stats]), ...]; every fragment is uploaded once per device and stays resident for the call."""
    pts = [_f64(f).reshape(-1, 3) for f in fragments]
    fts = [_f64(f) for f in features]
    if len(pts) != len(fts) or any(f.ndim != 2 or len(f) != len(p) for f, p in zip(fts, pts)):
        raise ValueError("one (N, dim) descriptor matrix per fragment")
    if not pairs:
        return []
    dim = fts[0].shape[1]
    if any(f.shape[1] != dim for f in fts):
        raise ValueError("every fragment must use descriptors of the same width")
    fv = (FragmentView * max(len(pts), 1))()
    for i, (p_, f_) in enumerate(zip(pts, fts)):
        fv[i].xyz, fv[i].feat, fv[i].n = _addr(p_), _addr(f_), len(p_)
    pr = (PairResult * len(pairs))()
    for k, (s_, t_) in enumerate(pairs):
        pr[k].s, pr[k].t = int(s_), int(t_)
        if seeds is not None and seeds[k] is not None:
            pr[k].seed, pr[k].has_seed = int(seeds[k]) & 0xFFFFFFFFFFFFFFFF, 1
    dev = (C.c_int * len(devices))(*[int(d) for d in devices])
    f = lib().m3d_register_fragment_pairs
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_double, C.c_double,
                  C.c_void_p, C.c_int, C.c_int]
    _check(f(C.cast(fv, C.c_void_p), len(pts), dim, C.cast(pr, C.c_void_p), len(pairs), float(voxel_size), int(max_iter),
             float(edge_length_threshold), float(confidence), C.cast(dev, C.c_void_p), len(devices), int(inflight)))
    out = []
    for k in range(len(pairs)):
        r = (pr[k].rc == 1, np.array(pr[k].T).reshape(4, 4), np.array(pr[k].info).reshape(6, 6))
        out.append(r + (pr[k].stats.asdict(),) if want_stats else r)
    return out


class RegSession:
    """m3d_reg: compute_transformation_ransac cut into begin_chunk / validate / replay (multi-GPU driver:
    misc3d_amd.distributed.registration_ransac_sharded).  Every rank must pass the same explicit seed."""

    def __init__(self, src, dst, corr_src, corr_dst, threshold=0.01, max_iter=100000, edge_length_threshold=0.9,
                 confidence=0.999, seed=0, device=0):
        src = _f64(src).reshape(-1, 3)
        dst = _f64(dst).reshape(-1, 3)
        cs = np.ascontiguousarray(corr_src, dtype=np.uint64)
        cd = np.ascontiguousarray(corr_dst, dtype=np.uint64)
        if len(cs) != len(cd):
            raise ValueError("correspondence lists differ in length")
        _s, sref = _seed_ref(seed)
        self._h = lib().m3d_reg_create(_p(src), len(src), _p(dst), len(dst), _p(cs), _p(cd), len(cs), threshold,
                                       max_iter, edge_length_threshold, confidence,
                                       C.cast(sref, C.c_void_p) if sref else None, device)
        if not self._h:
            msg = last_error()
            code = ERR_TOO_FEW_POINTS if "less than 3" in msg else (ERR_DEVICE if "HIP" in msg or "device" in msg
                                                                     else ERR_INVALID_ARG)
            raise M3DError(code, msg)

    def close(self):
        if getattr(self, "_h", None):
            lib().m3d_reg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def begin_chunk(self):
        """-> number of survivors of the next chunk, or None when the loop is over"""
        ns = C.c_size_t(0)
        rc = _check(lib().m3d_reg_begin_chunk(self._h, C.cast(C.byref(ns), C.c_void_p)))
        return int(ns.value) if rc == 1 else None

    def validate(self, s_begin, s_end):
        n = max(s_end - s_begin, 0)
        counts = np.zeros(max(n, 1), dtype=np.uint32)
        sums = np.zeros(max(n, 1), dtype=np.float64)
        _check(lib().m3d_reg_validate(self._h, s_begin, s_end, _p(counts), _p(sums)))
        return counts[:n], sums[:n]

    def replay(self, counts, sums):
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        sums = np.ascontiguousarray(sums, dtype=np.float64)
        if len(counts) == 0:
            counts, sums = np.zeros(1, dtype=np.uint32), np.zeros(1)
        _check(lib().m3d_reg_replay(self._h, _p(counts), _p(sums)))

    def finish(self):
        T = np.zeros(16)
        st = RegStats()
        _check(lib().m3d_reg_finish(self._h, _p(T), C.cast(C.byref(st), C.c_void_p)))
        return T.reshape(4, 4), st.asdict()


def match_last_fallbacks():
    return int(lib().m3d_match_last_fallbacks())


def match_mutual_nn(feat_src, feat_dst, method=1, n_trees=4, device=0):
    """feat_*: (N, dim) C-contiguous == Eigen dim x N column-major."""
    fs = _f64(feat_src)
    fd = _f64(feat_dst)
    if fs.ndim != 2 or fd.ndim != 2 or fs.shape[1] != fd.shape[1]:
        raise ValueError("descriptor matrices must be (N, dim) with equal dim")
    o0 = np.zeros(max(len(fs), 1), dtype=np.uint64)
    o1 = np.zeros(max(len(fs), 1), dtype=np.uint64)
    k = C.c_size_t(0)
    _check(lib().m3d_match_mutual_nn(_p(fs), len(fs), _p(fd), len(fd), fs.shape[1], method, n_trees, device, _p(o0),
                                     _p(o1), C.cast(C.byref(k), C.c_void_p)))
    return o0[: k.value].copy(), o1[: k.value].copy()


def replay(n_points, kind, max_iteration, probability, valid, counts, rmse=None):
    """Host-only replay of ransac.h:573-575,592-613 over gathered (valid, count) records."""
    st = ReplayState()
    lib().m3d_replay_init(C.byref(st))
    valid = np.ascontiguousarray(valid, dtype=np.uint8)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)

    def _cb(_user, i):
        return float(rmse(int(i))) if rmse is not None else 0.0

    cb = RMSE_FN(_cb)
    lib().m3d_replay_chunk(C.byref(st), n_points, kind, max_iteration, probability, 0, len(valid), _p(valid),
                           _p(counts), cb, None)
    return st
