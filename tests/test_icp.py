"""Point-to-plane ICP and multi-scale ICP, the part that needs no GPU: the argument checks of both entry points (decided before
any device work), the plain-C restatement (tests/cpp/icp_ref.c) against an independent numpy restatement, the guard on every
input the GPU tests use, and the stand-alone check of the 6 x 6 solve (tests/cpp/test_icp_solve.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import icp_ref_util as iu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return iu.IcpRef(tmp_path_factory.mktemp("icp_ref"))


@pytest.fixture(scope="module")
def tiny():
    p = iu.icp_pair(60, seed=3)
    return p["src"], p["dst"], p["dst_normals"]


def test_symbols_exported(capi):
    L = capi.lib()
    for name in ("m3d_registration_icp_plane", "m3d_multi_scale_icp"):
        assert hasattr(L, name), name
    assert C.sizeof(capi.MultiScaleIcpLevel) == 16 + C.sizeof(capi.IcpStats) + 24


def test_icp_plane_argument_checks_need_no_gpu(capi, tiny):
    src, dst, nrm = tiny
    with pytest.raises(capi.M3DError) as e:
        capi.registration_icp_plane(src, dst, None, 0.05)
    assert e.value.code == capi.ERR_INVALID_ARG and str(e.value) == "[Misc3D Error] " + iu.NO_NORMALS
    for d in (0.0, -1.0, float("nan")):
        with pytest.raises(capi.M3DError) as e:
            capi.registration_icp_plane(src, dst, nrm, d)
        assert e.value.code == capi.ERR_INVALID_ARG and str(e.value) == "[Misc3D Error] " + iu.INVALID_DISTANCE
    # Open3D checks the distance first
    with pytest.raises(capi.M3DError, match="Invalid max_correspondence_distance"):
        capi.registration_icp_plane(src, dst, None, 0.0)
    # null pointers
    L = capi.lib()
    assert L.m3d_registration_icp_plane(capi._p(src), len(src), capi._p(dst), capi._p(nrm), len(dst), 0.05, None, 30, 1e-6, 1e-6,
                                        0, None, None, None) == capi.ERR_INVALID_ARG
    # an empty cloud is no error and needs no device: the pose is the initial one, the first repeat meets both criteria
    init = iu.offset_pose(np.eye(4), 3.0, (0.1, 0.2, 0.3))
    T, st = capi.registration_icp_plane(np.zeros((0, 3)), dst, nrm, 0.05, init)
    assert np.array_equal(T, init) and st["iterations"] == 1 and st["converged"] == 1 and st["fitness"] == 0.0
    T, st, corr = capi.registration_icp_plane(src, np.zeros((0, 3)), np.zeros((0, 3)), 0.05, want_correspondences=True)
    assert np.array_equal(T, np.eye(4)) and np.all(corr == -1) and len(corr) == len(src)


def test_multi_scale_icp_argument_checks_need_no_gpu(capi, tiny):
    src, dst, nrm = tiny

    def fails(msg, *args, **kw):
        with pytest.raises(capi.M3DError) as e:
            capi.multi_scale_icp(*args, **kw)
        assert e.value.code == capi.ERR_INVALID_ARG and msg in str(e.value), str(e.value)

    fails("no levels", src, dst, [], [], 0.07, dst_normals=nrm)
    for method in (capi.REFINE_COLORED_ICP, capi.REFINE_GENERALIZED_ICP):
        fails("not accelerated", src, dst, [0.05], [50], 0.07, method=method, dst_normals=nrm)
    fails("Unknown local refine method.", src, dst, [0.05], [50], 0.07, method=7, dst_normals=nrm)
    fails(iu.NO_NORMALS, src, dst, [0.05], [50], 0.07, method=capi.REFINE_POINT2PLANE_ICP)
    for method, n in ((capi.REFINE_POINT2POINT_ICP, None), (capi.REFINE_POINT2PLANE_ICP, nrm)):
        for v in (0.0, -0.05, float("nan")):
            fails("[VoxelDownSample] voxel_size <= 0.", src, dst, [0.05, 0.025, v], [50, 30, 15], 0.07, method=method, dst_normals=n)
        fails("[VoxelDownSample] voxel_size is not finite.", src, dst, [0.05, float("inf")], [50, 30], 0.07, method=method,
              dst_normals=n)
        for d in (0.0, -0.07, float("nan")):
            fails(iu.INVALID_DISTANCE, src, dst, [0.05], [50], d, method=method, dst_normals=n)
    # the outputs of a refused call: the initial pose, a zero matrix
    L = capi.lib()
    init = iu.offset_pose(np.eye(4), 3.0, (0.1, 0.2, 0.3)).reshape(16).copy()
    T, info = np.full(16, 7.0), np.full(36, 7.0)
    assert L.m3d_multi_scale_icp(capi._p(src), None, len(src), capi._p(dst), None, len(dst), None, None, 0, 0.07, 0, capi._p(init), 0,
                                 capi._p(T), capi._p(info), None) == capi.ERR_INVALID_ARG
    assert np.array_equal(T, init) and not info.any()
    assert L.m3d_multi_scale_icp(capi._p(src), None, len(src), capi._p(dst), None, len(dst), None, None, 0, 0.07, 0, None, 0,
                                 None, capi._p(info), None) == capi.ERR_INVALID_ARG


def test_python_api_argument_checks_need_no_gpu(tiny):
    import misc3d_amd as m3d
    src, dst, nrm = tiny
    rec = m3d.reconstruction
    assert [(m.name, m.value) for m in rec.LocalRefineMethod] == [("Point2PointICP", 0), ("Point2PlaneICP", 1), ("ColoredICP", 2),
                                                                  ("GeneralizedICP", 3)]
    with pytest.raises(RuntimeError, match="require pre-computed normal"):
        m3d.registration_icp(src, dst, 0.05, estimation="point_to_plane")
    with pytest.raises(RuntimeError, match="estimation"):
        m3d.registration_icp(src, dst, 0.05, estimation="colored")
    with pytest.raises(RuntimeError, match="require pre-computed normal"):
        rec.refine_fragment_pair(src, dst, 0.05)
    with pytest.raises(RuntimeError, match="not accelerated"):
        rec.refine_fragment_pair(src, (dst, nrm), 0.05, method=rec.LocalRefineMethod.ColoredICP)
    with pytest.raises(RuntimeError, match="not accelerated"):
        rec.fragment_odometry(src, (dst, nrm), 0.05, method="generalized")
    with pytest.raises(RuntimeError, match="voxel_size <= 0"):
        rec.fragment_odometry(src, (dst, nrm), 0.0)
    with pytest.raises(RuntimeError, match="no levels"):
        rec.multi_scale_icp(src, (dst, nrm), [], [], 0.07)
    with pytest.raises(RuntimeError, match="Unknown local refine method"):
        rec.multi_scale_icp(src, (dst, nrm), [0.05], [50], 0.07, method="plane")


@pytest.mark.parametrize("name", ["small", "duplicates", "nonfinite", "no_correspondences"])
def test_c_reference_matches_the_numpy_restatement(ref, name):
    """brute-force search and numpy's solvers against the grid, the elimination and Horn's method of icp_ref.c, both estimators
    (two restatements that share no code agree to 1e-9 before either judges the GPU)"""
    c = iu.case(name)
    for nrm in (c["dst_normals"], None):
        a = ref.icp(c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"], nrm)
        with np.errstate(invalid="ignore"):
            b = iu.icp_numpy(c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"], nrm)
        assert a["iterations"] == b["iterations"] and a["converged"] == b["converged"]
        assert np.array_equal(a["corr"], b["corr"]) and a["fitness"] == b["fitness"]
        assert a["inlier_rmse"] == pytest.approx(b["inlier_rmse"], rel=1e-9, abs=0)
        assert np.allclose(a["T"], b["T"], rtol=0, atol=1e-9)


def test_reference_cases_have_the_properties_the_gpu_tests_name(ref):
    c = iu.case("refine")
    r = ref.icp(c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"], c["dst_normals"])
    assert r["converged"] == 1 and r["iterations"] >= 3 and np.allclose(r["T"], c["T"], rtol=0, atol=1e-3)
    c = iu.case("no_convergence")
    r = ref.icp(c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"], c["dst_normals"])
    assert r["converged"] == 0 and r["iterations"] == 2
    c = iu.case("duplicates")     # the tie is met, and the copy's normal would have moved the pose
    r = ref.icp(c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"], c["dst_normals"])
    n0 = len(c["dst"]) - 300
    assert np.all(r["corr"] < n0) and np.count_nonzero((r["corr"] >= 0) & (r["corr"] < 300)) > 100
    swapped_n = c["dst_normals"].copy()
    swapped_n[:300], swapped_n[n0:] = c["dst_normals"][n0:], c["dst_normals"][:300]
    other = ref.icp(c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"], swapped_n)
    assert np.abs(other["T"] - r["T"]).max() > 1e-6      # (a thousand times the GPU tests' pose tolerance)
    c = iu.case("nonfinite")
    r = ref.icp(c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"], c["dst_normals"])
    assert r["iterations"] == 1 and r["converged"] == 1 and np.array_equal(r["T"], c["init"])
    assert c["nan_normal_at"] in r["corr"] and r["corr"][3] == -1 and 0 < r["fitness"] < 1
    c = iu.case("no_correspondences")
    r = ref.icp(c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"], c["dst_normals"])
    assert r["fitness"] == 0.0 and np.array_equal(r["T"], c["init"]) and np.all(r["corr"] == -1)


def _guard(a, b):
    assert a["iterations"] == b["iterations"] and np.array_equal(a["corr"], b["corr"])
    assert np.allclose(a["T"], b["T"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", iu.CASES)
def test_input_guard_single_level(ref, name):
    """every input of the GPU tests: the reference summed in ascending and in descending index order gives the same iteration
    count and correspondences and poses within 1e-12 -- the order of the sums, which the device fixes differently, decides
    nothing on it.  An input that fails this is replaced, not tolerated."""
    c = iu.case(name)
    for nrm in (c["dst_normals"], None):
        _guard(ref.icp(c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"], nrm, order=1),
               ref.icp(c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"], nrm, order=-1))


@pytest.mark.parametrize("three", [True, False])
def test_input_guard_multi_scale(ref, three):
    m = iu.multi_case()
    vs, its = iu.levels_of(m["voxel"], three)
    for nrm in (m["dst_normals"], None):
        a = ref.multi_scale(m["src"], m["dst"], vs, its, m["max_dist"], m["init"], nrm, order=1)
        b = ref.multi_scale(m["src"], m["dst"], vs, its, m["max_dist"], m["init"], nrm, order=-1)
        for x, y in zip(a["levels"], b["levels"]):
            _guard(x, y)
        assert a["n_info"] == b["n_info"]
        assert a["levels"][0]["iterations"] >= 3       # the first level has work to do
        if nrm is not None:
            assert np.allclose(a["T"], m["T"], rtol=0, atol=1e-3)


def test_icp_solve_is_pinned_on_the_host(tmp_path):
    """tests/cpp/test_icp_solve.cpp compiles misc3d_amd/csrc/m3d_icp_fp.hpp -- the text the library compiles -- with g++: the
    identity for an empty, singular or NaN system, a hand-computed case, the rotation order, the LDL^T residual."""
    exe = str(tmp_path / "test_icp_solve")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "test_icp_solve.cpp"),
                    "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK") and "FAILED" not in r.stdout, r.stdout + r.stderr
