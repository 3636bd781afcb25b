"""misc3d.preprocessing without a GPU: the C restatement of FarthestPointSampling (tests/cpp/fps_ref.c) against a numpy
one, what the seam clouds of the GPU tests promise (fps_ref_util.py), shown from the two restatements alone, the early cases of m3d_farthest_point_sampling (decided before any device is touched), CropROIPointCloud's index
formula (m3d_crop_roi_indices, host only), the exported symbols, and the pruned path's tile bound on the host
(tests/cpp/test_fps_bound.cpp over misc3d_amd/csrc/m3d_fps_fp.hpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from fps_ref_util import (FPS_CROSSOVER, FPS_SINGLE_SEAMS, FPS_TILE, build_ref, fps_numpy, fps_seam_cloud, fps_tie_steps,
                          fps_tile_edge_cloud, fps_unsorted_clouds, quirk_clouds, shaped_clouds)

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("fps_ref"))


@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_matches_numpy_on_shaped_clouds(ref, seed):
    for name, pts in shaped_clouds(700, seed).items():
        for S in (1, 2, 50, len(pts) - 1):
            assert np.array_equal(ref(pts, S), fps_numpy(pts, S)), (name, S)


def test_restatement_matches_numpy_on_quirk_clouds(ref):
    for name, pts in quirk_clouds().items():
        for S in (1, 3, 40, len(pts) - 1):
            assert np.array_equal(ref(pts, S), fps_numpy(pts, S)), (name, S)


def test_restatement_quirks(ref):
    q = quirk_clouds()
    assert not ref(q["all_equal"], 10).any()                       # nothing > 0: index 0 again and again
    k = ref(q["k_distinct"], 12)
    assert len(set(k[:5].tolist())) == 5 and (k[5:] == k[4]).all()  # k distinct positions, then the last index repeats
    assert not ref(q["nan_first"], 20).any()                        # NaN at index 0: 0 forever
    nf = ref(q["nonfinite_later"], 30)                              # the lowest non-finite index wins at step 1, then stays
    assert nf[0] == 0 and (nf[1:] == 17).all()
    ov = ref(q["overflow"], 8)
    assert len(set(ov.tolist())) == 8


@pytest.mark.parametrize("n", FPS_SINGLE_SEAMS + (FPS_CROSSOVER,))
def test_seam_cloud_selects_its_last_two_points(ref, n):
    """what the GPU seam tests rely on: the two points at the end of the input are among the first three samples, so a
    kernel that loses its highest register slot, its last lane or its last tile cannot agree with the restatement"""
    pts = fps_seam_cloud(n, n)
    got = ref(pts, 64)
    assert got[0] == 0 and {n - 1, n - 2} == set(got[1:3].tolist())
    assert len(set(got.tolist())) == 64
    assert np.array_equal(got, fps_numpy(pts, 64))
    for S in (2, 3):
        assert np.array_equal(ref(pts, S), got[:S])


@pytest.mark.parametrize("n", [2049, 4097])
def test_lattice_clouds_have_ties(ref, n):
    """the lattice clouds of the GPU tie tests: at some steps several points hold the largest distance exactly"""
    pts = shaped_clouds(n)["lattice"]
    assert len(pts) == n
    assert fps_tie_steps(pts, 500) >= 10
    assert np.array_equal(ref(pts, 500), fps_numpy(pts, 500))


def test_unsorted_layout_clouds(ref):
    """the extents no sorting grid can take, and what the restatement gives on them"""
    clouds = fps_unsorted_clouds()
    with np.errstate(over="ignore", invalid="ignore"):
        for name, pts in clouds.items():
            assert pts.shape == (9001, 3)
            fin = pts[np.isfinite(pts).all(axis=1)]
            ext = (fin.max(axis=0) - fin.min(axis=0)).max()
            assert np.isinf(ext) if name != "subnormal_extent" else 0 < ext < 1e-290, name
            assert np.array_equal(ref(pts, 40), fps_numpy(pts, 40)), name
    a = ref(clouds["inf_extent"], 40)
    assert a[:3].tolist() == [0, 100, 7000] and len(set(a.tolist())) == 40
    b = ref(clouds["inf_extent_nonfinite"], 40)
    assert b[:2].tolist() == [0, 100] and (b[2:] == 5000).all()
    assert not ref(clouds["subnormal_extent"], 40).any()


@pytest.mark.parametrize("n_finite", [20 * FPS_TILE, 20 * FPS_TILE + 1])
def test_tile_edge_clouds(ref, n_finite):
    full = fps_tile_edge_cloud(n_finite, 0, 3)
    assert len(full) == n_finite and np.isfinite(full).all()
    assert np.array_equal(ref(full, 64), fps_numpy(full, 64))
    pts = fps_tile_edge_cloud(n_finite, 3, 3)
    rows = np.nonzero(~np.isfinite(pts).all(axis=1))[0]
    assert len(pts) == n_finite + 3 and len(rows) == 3 and rows[0] > 0
    got = ref(pts, 64)
    assert got[0] == 0 and (got[1:] == rows[0]).all()       # the lowest non-finite index at step 1, then for ever
    assert np.array_equal(got, fps_numpy(pts, 64))


def test_restatement_orders_differ_only_in_association(tmp_path):
    r0, r1 = build_ref(tmp_path, 0), build_ref(tmp_path, 1)
    pts = shaped_clouds(400, 3)["cube"]
    a, b = r0(pts, 100), r1(pts, 100)
    assert a[0] == b[0] == 0 and len(set(b.tolist())) == 100


def _fps_status(capi, xyz, S):
    try:
        return capi.farthest_point_sampling(xyz, S), None
    except capi.M3DError as e:
        return None, str(e)


def test_fps_early_cases_without_device(capi):
    pts = np.random.default_rng(0).uniform(-1, 1, (37, 3))
    idx, err = _fps_status(capi, pts, 0)
    assert err is None and len(idx) == 0
    idx, err = _fps_status(capi, pts, 37)
    assert err is None and np.array_equal(idx, np.arange(37))
    idx, err = _fps_status(capi, np.zeros((0, 3)), 0)
    assert err is None and len(idx) == 0
    _, err = _fps_status(capi, pts, 38)
    assert err == "[Misc3D Error] Illegal number of samples: 38, must <= point size: 37"
    _, err = _fps_status(capi, pts, -3)
    assert err == "[Misc3D Error] Illegal number of samples: -3, must <= point size: 37"
    _, err = _fps_status(capi, np.zeros((0, 3)), 1)
    assert err == "[Misc3D Error] Illegal number of samples: 1, must <= point size: 0"
    st = capi.farthest_point_sampling(pts, 37, stats=True)[1]
    assert st["path"] == 0 and st["ms_device"] == 0.0


def test_python_api_early_cases_and_project_into_plane():
    import misc3d_amd as m3d
    pts = np.random.default_rng(1).uniform(-1, 1, (9, 3))

    class Obj:
        points = pts
    assert m3d.preprocessing.farthest_point_sampling(Obj(), 9) == list(range(9))
    a = m3d.preprocessing.farthest_point_sampling(pts, 9, as_arrays=True)
    assert a.dtype == np.int64 and np.array_equal(a, np.arange(9))
    assert m3d.preprocessing.farthest_point_sampling(pts, 0) == []
    with pytest.raises(RuntimeError, match=r"Illegal number of samples: 10, must <= point size: 9"):
        m3d.preprocessing.farthest_point_sampling(pts, 10)
    with pytest.raises(RuntimeError, match="project_into_plane"):
        m3d.preprocessing.project_into_plane(pts)


def _crop_formula(roi, shape):
    tl_x, tl_y, br_x, br_y = roi
    width, _ = shape
    w, h = br_x - tl_x, br_y - tl_y
    return np.array([(i // w + tl_y) * width + (i % w) + tl_x for i in range((w + 1) * (h + 1))], dtype=np.uint64)


def test_crop_roi_indices_formula(capi):
    shape = (40, 30)
    n = shape[0] * shape[1]
    for roi in [(3, 4, 10, 9), (0, 0, 1, 0), (5, 5, 20, 5), (0, 0, 39, 26), (10, 2, 11, 12)]:
        got = capi.crop_roi_indices(n, roi, shape)
        exp = _crop_formula(roi, shape)
        assert np.array_equal(got, exp), roi
        w, h = roi[2] - roi[0], roi[3] - roi[1]
        assert len(got) == (w + 1) * (h + 1)   # the reference's count: rows w wide, (w + 1) (h + 1) of them
    assert len(capi.crop_roi_indices(n, (3, 4, 10, 3), shape)) == 0   # roi_h = -1: (h + 1) = 0 points


def test_crop_roi_errors(capi):
    with pytest.raises(capi.M3DError, match=r"^\[Misc3D Error\] The size of point cloud is wrong\.$"):
        capi.crop_roi_indices(100, (0, 0, 2, 2), (10, 9))
    with pytest.raises(capi.M3DError, match="br_x"):
        capi.crop_roi_indices(100, (5, 0, 5, 2), (10, 10))   # roi_w = 0: the reference divides by zero
    with pytest.raises(capi.M3DError, match="br_x"):
        capi.crop_roi_indices(100, (6, 0, 5, 2), (10, 10))
    with pytest.raises(capi.M3DError, match="outside the cloud"):
        capi.crop_roi_indices(100, (0, 5, 9, 9), (10, 10))  # (w + 1)(h + 1) reaches row 10
    with pytest.raises(capi.M3DError, match="outside the cloud"):
        capi.crop_roi_indices(100, (-2, 0, 3, 1), (10, 10))


def test_crop_roi_pointcloud_python():
    import misc3d_amd as m3d
    pts = np.arange(4 * 3 * 3, dtype=np.float64).reshape(12, 3)
    out = m3d.preprocessing.crop_roi_pointcloud(pts, (1, 0, 3, 1), (4, 3))
    got = np.asarray(getattr(out, "points", out))
    assert np.array_equal(got, pts[_crop_formula((1, 0, 3, 1), (4, 3)).astype(np.int64)])
    with pytest.raises(RuntimeError, match="The size of point cloud is wrong"):
        m3d.preprocessing.crop_roi_pointcloud(pts, (0, 0, 1, 1), (5, 3))


def test_preprocessing_symbols_exported(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in ("m3d_farthest_point_sampling", "m3d_crop_roi_indices", "m3d_bench_fps_force_path"):
        assert hasattr(L, name), name
    hdr = open(capi.HEADER_PATH).read()
    assert "m3d_fps_stats" in hdr and "m3d_farthest_point_sampling" in hdr and "m3d_crop_roi_indices" in hdr
    for order in ("order1", "order2"):
        p = os.path.join(os.path.dirname(capi.LIB_PATH), order, "libmisc3d_amd.so")
        if os.path.exists(p):
            assert hasattr(ctypes.CDLL(p), "m3d_farthest_point_sampling"), order


def test_fps_tile_bound_host(tmp_path):
    exe = str(tmp_path / "test_fps_bound")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(HERE, "cpp", "test_fps_bound.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe, "1000000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "triples=1000000 violations=0" in r.stdout
