"""Ray casting without a GPU: the plain-C brute force (tests/cpp/raycast_ref.c) against an independent numpy float32
restatement of the contract, the host check of the kernels' arithmetic (tests/cpp/test_raycast_fp.cpp), and the module, the
class, the symbol and the argument checks of m3d_raycast_pinhole, all of which need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import raycast_ref_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp("raycast_ref"))


@pytest.mark.parametrize("name", list(U.scenes()))
def test_checker_equals_numpy_restatement(ref, name):
    """every scene the GPU is judged on: the two restatements agree bit for bit before either judges the device"""
    meshes, poses, cam, hits = U.scenes()[name]
    a, b = ref(meshes, poses, cam), U.raycast_numpy(meshes, poses, cam)
    assert U.same(a, b), U.first_difference(a, b)
    assert bool(np.isfinite(a["t_hit"]).any()) == hits


def test_checker_equals_numpy_on_the_batch_frames(ref):
    for poses in U.BATCH_FRAMES():
        a, b = ref(U.BATCH_MESHES(), poses, U.CAM), U.raycast_numpy(U.BATCH_MESHES(), poses, U.CAM)
        assert U.same(a, b), U.first_difference(a, b)


def test_checker_rules(ref):
    """rule 4's ties and misses, t as the z-depth, the normal's orientation"""
    quad = (np.array([[-1.0, -1.0, 2.0], [1.0, -1.0, 2.0], [1.0, 1.0, 2.0], [-1.0, 1.0, 2.0]]), np.array([[0, 1, 2], [0, 2, 3]]))
    r = ref([quad, quad], [U.identity(), U.identity()], U.CAM)
    hit = np.isfinite(r["t_hit"])
    assert hit.any() and not hit.all()
    assert np.all(r["t_hit"][hit] == np.float32(2.0))                 # not the distance along the ray
    assert np.all(r["geometry_ids"][hit] == 0)                        # equal t: the lowest geometry id
    assert np.all(r["geometry_ids"][~hit] == U.INVALID) and np.all(r["primitive_ids"][~hit] == U.INVALID)
    assert np.all(r["t_hit"][~hit] == np.inf) and np.all(r["normals"][~hit] == 0)
    assert np.all(r["normals"][hit] == np.array([0, 0, 1], np.float32))   # (v1 - v0) x (v2 - v0), not turned to the camera
    # the diagonal belongs to both triangles: the lower primitive id wins there
    W, H, fx, fy, cx, cy = 65, 65, 32.0, 32.0, 32.5, 32.5
    d = ref([quad], [U.identity()], (W, H, fx, fy, cx, cy))
    on_diagonal = np.diag(d["primitive_ids"])
    assert np.all(on_diagonal[np.isfinite(np.diag(d["t_hit"]))] == 0) and (on_diagonal == 0).sum() > 30
    assert (d["primitive_ids"] == 1).any()
    with pytest.raises(U.RefNonFinite) as e:
        ref([quad], [np.diag([1e39, 1.0, 1.0, 1.0])], U.CAM)
    assert e.value.index == 0
    with pytest.raises(U.RefNonFinite):
        U.raycast_numpy([quad], [np.diag([1e39, 1.0, 1.0, 1.0])], U.CAM)


def test_reference_example_clause_rejects_nothing(ref):
    """the reference's example scene at a sixteenth of its resolution: the culling clause of rule 3 rejects no
    Moeller-Trumbore hit and both instances are seen (the GPU test repeats this at a quarter)"""
    mesh, poses, cam = U.golden_obj(16)
    r = ref([mesh, mesh], poses, cam)
    again = U.raycast_numpy([mesh, mesh], poses, cam, rows_per_chunk=2)
    assert U.same(r, again), U.first_difference(r, again)
    assert r["counts"]["mt_hits"] > 0 and r["counts"]["clause_rejected"] == 0 and r["counts"]["pixels_changed"] == 0
    assert set(np.unique(r["geometry_ids"])) == {0, 1, U.INVALID}


def test_fp_header_host_check(tmp_path):
    """tests/cpp/test_raycast_fp.cpp: nested boxes give nested slabs and ordered lower bounds, no box around an accepted
    triangle is culled, and rule 3 equals the C restatement pair by pair"""
    obj, exe = str(tmp_path / "raycast_ref.o"), str(tmp_path / "test_raycast_fp")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-c", os.path.join(ROOT, "tests", "cpp", "raycast_ref.c"), "-o", obj], check=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "test_raycast_fp.cpp"), obj,
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ---- the library: what needs no device ---------------------------------------------------------------------------------------
def test_module_class_and_symbol_exist(capi):
    import misc3d_amd as m3d
    assert hasattr(capi.lib(), "m3d_raycast_pinhole")
    assert C.sizeof(capi.RaycastStats) == 80 and C.sizeof(capi.RaycastMesh) == 32
    assert "m3d_raycast_pinhole" in open(capi.HEADER_PATH).read()
    r = m3d.pose_estimation.RayCastRenderer(U.CAM)
    for name in ("cast_rays", "cast_rays_batch", "get_depth_map", "get_instance_map", "get_primitive_ids", "get_normal_map",
                 "get_point_cloud", "get_instance_point_cloud"):
        assert callable(getattr(r, name)), name
    assert "pose_estimation" in m3d.__all__
    assert os.path.exists(os.path.join(ROOT, "include", "misc3d", "pose_estimation", "ray_cast_renderer.h"))


class _Intrinsic:   # the shape of open3d.camera.PinholeCameraIntrinsic
    width, height = 64, 48
    intrinsic_matrix = np.array([[60.0, 0, 31.5], [0, 61.0, 23.5], [0, 0, 1]])


class _Mesh:        # the shape of open3d.geometry.TriangleMesh
    def __init__(self, v, f):
        self.vertices, self.triangles = v, f


@pytest.fixture
def warnings_on():
    """the warnings follow the verbosity level, which other tests of the session may have lowered"""
    import misc3d_amd as m3d
    before = m3d.get_verbosity_level()
    m3d.set_verbosity_level(m3d.Info)
    yield
    m3d.set_verbosity_level(before)


def test_empty_list_getters_and_numpy_shim(capi, capsys, warnings_on):
    import misc3d_amd as m3d
    r = m3d.pose_estimation.RayCastRenderer(_Intrinsic())
    assert r._cam == (64, 48, 60.0, 61.0, 31.5, 23.5)
    assert r.cast_rays([], []) is False
    assert "[Misc3D WARNING] No mesh is provided." in capsys.readouterr().out
    assert capi.raycast_pinhole([], [[]], U.CAM) is None and capi.last_error() == "No mesh is provided."
    depth, inst = r.get_depth_map(), r.get_instance_map()
    assert capsys.readouterr().out.count("[Misc3D WARNING] No ray cast result is available.") == 2
    assert depth.size == 0 and inst.size == 0 and depth.dtype == np.float32 and inst.dtype == np.uint32
    assert isinstance(depth, np.ndarray) and depth.numpy() is depth and inst.numpy() is inst
    pts, nrm = r.get_point_cloud()
    assert pts.shape == (0, 3) and nrm.shape == (0, 3) and r.get_instance_point_cloud() == []
    assert r.get_primitive_ids().size == 0 and r.get_normal_map().size == 0
    assert r.cast_rays_batch([], []) is None
    m3d.set_verbosity_level(m3d.Error)          # ... and are silent below Warning, as the reference's
    capsys.readouterr()
    assert r.cast_rays([], []) is False and r.get_depth_map().size == 0 and capsys.readouterr().out == ""


def test_argument_errors_need_no_gpu(capi):
    import misc3d_amd as m3d
    v, f = U.sphere(4, 5)
    r = m3d.pose_estimation.RayCastRenderer(U.CAM)
    with pytest.raises(RuntimeError) as e:
        r.cast_rays([_Mesh(v, f), (v, f)], [np.eye(4)])
    assert str(e.value) == "[Misc3D Error] The number of meshes and poses are not matched."
    with pytest.raises(capi.M3DError) as e:
        capi.raycast_pinhole([(v, f)], [[np.eye(4), np.eye(4)]], U.CAM)
    assert e.value.code == capi.ERR_SIZE_MISMATCH

    def refused(meshes, poses, cam, text):
        with pytest.raises(capi.M3DError) as e:
            capi.raycast_pinhole(meshes, [poses], cam, outputs=())   # (no maps: nothing is allocated for a refused size)
        assert e.value.code == capi.ERR_INVALID_ARG and text in str(e.value), str(e.value)

    bad_f = f.copy()
    bad_f[3, 1] = len(v)
    refused([(v, f), (v, bad_f)], [np.eye(4)] * 2, U.CAM, "triangle 3 of mesh 1 has a vertex index out of range")
    bad_f[3, 1] = -1
    refused([(v, bad_f)], [np.eye(4)], U.CAM, "vertex index out of range")
    for bad in (np.nan, np.inf):
        bad_v = v.copy()
        bad_v[2, 0] = bad
        refused([(v, f), (bad_v, f)], [np.eye(4)] * 2, U.CAM, "vertex 2 of mesh 1 is not finite")
        T = np.eye(4)
        T[1, 3] = bad
        refused([(v, f)], [T], U.CAM, "pose 0 of frame 0 is not finite")
        for k in range(2, 6):
            cam = list(U.CAM)
            cam[k] = bad
            refused([(v, f)], [np.eye(4)], tuple(cam), "intrinsic parameters are not finite")
    refused([(v, f)], [np.eye(4)], (0, 48, 60.0, 60.0, 31.5, 23.5), "width and height")
    refused([(v, f)], [np.eye(4)], (64, -3, 60.0, 60.0, 31.5, 23.5), "width and height")
    refused([(v, f)], [np.eye(4)], (64, 48, 0.0, 60.0, 31.5, 23.5), "fx and fy must not be 0")
    refused([(v, f)], [np.eye(4)], (64, 48, 60.0, -0.0, 31.5, 23.5), "fx and fy must not be 0")
    refused([(v, f)], [np.eye(4)], (64, 48, 1e-300, 60.0, 31.5, 23.5), "ray direction is not finite")
    refused([(v, f)], [np.eye(4)], (65536, 32768, 60.0, 60.0, 31.5, 23.5), "too many pixels")
    # the second frame's poses are checked as well, before anything runs
    T = np.eye(4)
    T[0, 0] = np.nan
    with pytest.raises(capi.M3DError) as e:
        capi.raycast_pinhole([(v, f)], [[np.eye(4)], [T]], U.CAM)
    assert "pose 0 of frame 1 is not finite" in str(e.value)
    # null pointers
    L = capi.lib()
    mesh = capi.RaycastMesh(None, 3, None, 1)
    assert L.m3d_raycast_pinhole(C.cast(C.byref(mesh), C.c_void_p), 1, capi._p(np.eye(4)), 1, 1, 64, 48, 60.0, 60.0, 31.5, 23.5, 0,
                                 None, None, None, None, None) == capi.ERR_INVALID_ARG
    # no frames: nothing to do, no device needed
    assert capi.raycast_pinhole([(v, f)], [], U.CAM)["t_hit"].shape == (0, 48, 64)


def test_no_device_is_an_error(capi):
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    v, f = U.sphere(4, 5)
    with pytest.raises(capi.M3DError) as e:
        capi.raycast_pinhole([(v, f)], [[np.eye(4)]], U.CAM)
    assert e.value.code == capi.ERR_DEVICE
    import misc3d_amd as m3d
    with pytest.raises(RuntimeError, match="no HIP device"):
        m3d.pose_estimation.RayCastRenderer(U.CAM).cast_rays([(v, f)], [np.eye(4)])
