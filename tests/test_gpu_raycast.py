"""Ray casting on the GPU (m3d_raycast_pinhole, pose_estimation.RayCastRenderer): every case compares the four maps with the
plain-C brute force (tests/cpp/raycast_ref.c) bit for bit -- the trees of 1, 2 and 255 / 256 / 257 triangles, equal Morton
codes, equal hits from two meshes, an empty mesh, triangles at and behind z = 0 and around the origin, slivers, overflowing
products, a column with dx == 0, images that are no multiple of the ray tile, many meshes, batches, repeats, the Python
class, the C++ mirror, and the reference's example scene at a quarter of its resolution."""
import os
import struct
import subprocess

import numpy as np
import pytest

import raycast_ref_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev(capi):
    if capi.device_count() < 1:
        pytest.skip("needs an MI355X")
    return 0


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp("raycast_ref"))


def gpu(capi, meshes, poses, cam, **kw):
    r = capi.raycast_pinhole(meshes, [poses], cam, **kw)
    if isinstance(r, tuple):
        return {k: v[0] for k, v in r[0].items()}, r[1]
    return {k: v[0] for k, v in r.items()}


def check(capi, ref, meshes, poses, cam):
    got, exp = gpu(capi, meshes, poses, cam), ref(meshes, poses, cam)
    assert U.same(got, exp), U.first_difference(got, exp)
    return got, exp


SCENES = U.scenes()


def scene(capi, ref, name):
    meshes, poses, cam, hits = SCENES[name]
    got, exp = check(capi, ref, meshes, poses, cam)
    assert bool(np.isfinite(got["t_hit"]).any()) == hits
    return got


@pytest.mark.parametrize("name", ["1 triangle", "1 triangle, posed", "2 triangles", "2 meshes of 1 triangle", "255 triangles",
                                  "256 triangles", "257 triangles", "crossing z = 0", "behind, crossing, in front",
                                  "around the origin", "origin triangles and a sphere", "slivers and zero area",
                                  "1e30, 1e-30 and 1", "dx = 0 and dy = 0", "1 x 1", "7 x 5", "65 x 9", "40 small meshes"])
def test_scene_equals_brute_force(capi, dev, ref, name):
    """the trees of one and two triangles, sizes around a workgroup, triangles through and around the camera, slivers and
    zero-area triangles in a sphere, products that overflow and underflow, images off the 8 x 8 ray tile, many meshes"""
    scene(capi, ref, name)


def test_identical_triangles_equal_codes(capi, dev, ref):
    """300 copies of one triangle: every Morton code is equal, the tree is as deep as the position bits make it, and every
    hit must name primitive 0"""
    got = scene(capi, ref, "300 identical triangles")
    assert np.all(got["primitive_ids"][np.isfinite(got["t_hit"])] == 0)


def test_identical_meshes_name_geometry_zero(capi, dev, ref):
    got = scene(capi, ref, "identical meshes, same pose")
    assert np.all(got["geometry_ids"][np.isfinite(got["t_hit"])] == 0)


def test_empty_mesh_keeps_its_id(capi, dev, ref):
    got = scene(capi, ref, "empty mesh between")
    assert set(np.unique(got["geometry_ids"])) == {0, 2, U.INVALID}
    got = scene(capi, ref, "only empty meshes")
    assert np.all(got["t_hit"] == np.inf) and np.all(got["geometry_ids"] == U.INVALID) and np.all(got["normals"] == 0)


@pytest.mark.parametrize("name", ["behind the camera", "through the origin", "1e30", "1e-30"])
def test_nothing_is_hit(capi, dev, ref, name):
    got = scene(capi, ref, name)
    assert np.all(got["t_hit"] == np.inf) and np.all(got["primitive_ids"] == U.INVALID)


def test_a_vertex_that_overflows_is_refused(capi, dev, ref):
    with pytest.raises(capi.M3DError) as e:
        gpu(capi, [U.TRI, U.TRI], [U.identity(), np.diag([1.0, 1e39, 1.0, 1.0])], U.CAM)
    assert e.value.code == capi.ERR_NON_FINITE and "vertex 3 of the mesh list (mesh 1)" in str(e.value)
    with pytest.raises(U.RefNonFinite) as r:
        ref([U.TRI, U.TRI], [U.identity(), np.diag([1.0, 1e39, 1.0, 1.0])], U.CAM)
    assert r.value.index == 3


def test_a_column_with_dx_zero(capi, dev, ref):
    cam = SCENES["dx = 0"][2]
    assert np.float32(((32 + 0.5) - cam[4]) / cam[2]) == 0
    scene(capi, ref, "dx = 0")


def test_batch_equals_single_calls_and_repeats(capi, dev, ref):
    meshes, frames = U.BATCH_MESHES(), U.BATCH_FRAMES()
    batch, st = capi.raycast_pinhole(meshes, frames, U.CAM, stats=True)
    assert batch["t_hit"].shape == (3, 48, 64) and batch["normals"].shape == (3, 48, 64, 3)
    for k in range(3):
        one = gpu(capi, meshes, frames[k], U.CAM)
        frame = {key: batch[key][k] for key in U.KEYS}
        assert U.same(frame, one), (k, U.first_difference(frame, one))
        exp = ref(meshes, frames[k], U.CAM)
        assert U.same(frame, exp), (k, U.first_difference(frame, exp))
    again = capi.raycast_pinhole(meshes, frames, U.CAM)
    assert U.same(again, batch)
    n_tri = sum(len(m[1]) for m in meshes)
    assert st["n_triangles"] == n_tri and st["n_nodes"] == 2 * n_tri - 1 and st["n_rays"] == 3 * 64 * 48
    assert 0 < st["pair_tests"] < st["n_rays"] * n_tri and st["nodes_visited"] >= st["n_rays"]
    assert st["ms_total"] > 0 and st["ms_build"] > 0 and st["ms_traverse"] > 0
    # only the maps that are asked for
    only = capi.raycast_pinhole(meshes, frames[:1], U.CAM, outputs=("geometry_ids",))
    assert list(only) == ["geometry_ids"] and np.array_equal(only["geometry_ids"][0], batch["geometry_ids"][0])


class _Intrinsic:
    def __init__(self, cam):
        self.width, self.height = cam[0], cam[1]
        self.intrinsic_matrix = np.array([[cam[2], 0, cam[4]], [0, cam[3], cam[5]], [0, 0, 1]])


class _Mesh:
    def __init__(self, v, f):
        self.vertices, self.triangles = v, f


def test_python_class(capi, dev, ref):
    import misc3d_amd as m3d
    meshes = [U.sphere(8, 12, 0.3, (-0.3, 0, 2)), U.sphere(8, 12, 0.3, (0.3, 0, 2.2))]
    poses = [U.identity(), U.pose(0.2, 0.0, 0.0)]
    exp = ref(meshes, poses, U.CAM)
    r = m3d.pose_estimation.RayCastRenderer(_Intrinsic(U.CAM))
    assert r.cast_rays([_Mesh(*meshes[0]), meshes[1]], poses) is True
    depth, inst = r.get_depth_map().numpy(), r.get_instance_map().numpy()       # as the reference's example reads them
    got = {"t_hit": depth, "geometry_ids": inst, "primitive_ids": r.get_primitive_ids(), "normals": r.get_normal_map()}
    assert depth.shape == (48, 64) and depth.dtype == np.float32 and inst.dtype == np.uint32
    assert U.same(got, exp), U.first_difference(got, exp)
    W, H, fx, fy, cx, cy = U.CAM
    d = np.stack(np.broadcast_arrays((((np.arange(W) + 0.5) - cx) / fx).astype(np.float32)[None, :],
                                     (((np.arange(H) + 0.5) - cy) / fy).astype(np.float32)[:, None], np.float32(1.0)), axis=-1)
    hit = np.isfinite(exp["t_hit"])
    pts, nrm = r.get_point_cloud()
    assert pts.dtype == np.float64 and np.array_equal(pts, (d[hit] * exp["t_hit"][hit][:, None]).astype(np.float64))
    assert np.array_equal(nrm, exp["normals"][hit].astype(np.float64))
    clouds = r.get_instance_point_cloud()
    assert len(clouds) == 2
    for i, (p, n) in enumerate(clouds):
        m = exp["geometry_ids"] == i
        assert m.any() and np.array_equal(p, (d[m] * exp["t_hit"][m][:, None]).astype(np.float64))
        assert np.array_equal(n, exp["normals"][m].astype(np.float64))
    batch = r.cast_rays_batch(meshes, [poses, poses])
    assert batch["t_hit"].shape == (2, 48, 64) and U.same({k: batch[k][1] for k in U.KEYS}, exp)


def test_cpp_mirror(capi, dev, ref, tmp_path):
    exe = str(tmp_path / "raycast_mirror")
    lib = os.path.join(ROOT, "misc3d_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_raycast_mirror.cpp"), "-o", exe, "-L", lib, "-lmisc3d_amd", "-lpthread",
                    "-Wl,-rpath," + lib], check=True)
    meshes = [U.as_mesh(U.sphere(8, 12, 0.3, (-0.3, 0, 2))), U.as_mesh(U.sphere(8, 12, 0.3, (0.3, 0, 2.2)))]
    poses = [U.identity(), U.pose(0.2, 0.0, 0.0)]
    W, H, fx, fy, cx, cy = U.CAM
    blob = tmp_path / "scene.bin"
    with open(blob, "wb") as f:
        f.write(struct.pack("<qqddddq", W, H, fx, fy, cx, cy, len(meshes)))
        for (v, t), T in zip(meshes, poses):
            f.write(struct.pack("<qq", len(v), len(t)))
            f.write(v.tobytes())
            f.write(t.tobytes())
            f.write(np.ascontiguousarray(T, dtype=np.float64).tobytes())
    r = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    at = 0

    def take():
        nonlocal at
        at += 1
        return lines[at - 1]

    for _ in range(4):
        assert take() == "[Misc3D WARNING] No ray cast result is available."
    assert take() == "before 0 0 0 0"
    assert take() == "[Misc3D WARNING] No mesh is provided." and take() == "empty 0"
    assert take() == "[Misc3D Error] The number of meshes and poses are not matched."
    assert take() == "cast 1" and take() == f"maps {W * H}"
    exp = ref(meshes, poses, U.CAM)
    maps = np.array([[int(x, 16) for x in take().split()] for _ in range(W * H)], dtype=np.uint64).reshape(H, W, 3)
    assert np.array_equal(maps[..., 0], U.bits32(exp["t_hit"])) and np.array_equal(maps[..., 1], exp["geometry_ids"])
    assert np.array_equal(maps[..., 2], exp["primitive_ids"])
    d = np.stack(np.broadcast_arrays((((np.arange(W) + 0.5) - cx) / fx).astype(np.float32)[None, :],
                                     (((np.arange(H) + 0.5) - cy) / fy).astype(np.float32)[:, None], np.float32(1.0)), axis=-1)

    def cloud(tag, mask):
        n = int(mask.sum())
        assert take() == f"{tag} {n} {n}"
        rows = np.array([[int(x, 16) for x in take().split()] for _ in range(n)], dtype=np.uint64).reshape(n, 6)
        pts = (d[mask] * exp["t_hit"][mask][:, None]).astype(np.float64)
        assert np.array_equal(rows[:, :3], pts.view(np.uint64)) and np.array_equal(rows[:, 3:], exp["normals"][mask].astype(np.float64).view(np.uint64))

    cloud("cloud", np.isfinite(exp["t_hit"]))
    assert take() == "instances 2"
    for i in range(2):
        cloud("instance", exp["geometry_ids"] == i)


def test_reference_example_scene(capi, dev, tmp_path_factory):
    """the reference's ray_cast_rendering example (obj.ply scaled by 0.001 at its two poses) at 160 x 120 with the example's
    intrinsics divided by 4: bit for bit the brute force; the culling clause of rule 3 rejects no Moeller-Trumbore hit; both
    instances are seen"""
    ref = U.build_ref(tmp_path_factory.mktemp("raycast_ref_omp"), openmp=True)   # 448 M pairs: the rows shared among threads
    mesh, poses, cam = U.golden_obj(4)
    assert cam[:2] == (160, 120) and len(mesh[1]) == 11678
    got, st = gpu(capi, [mesh, mesh], poses, cam, stats=True)
    exp = ref([mesh, mesh], poses, cam)
    assert U.same(got, exp), U.first_difference(got, exp)
    assert exp["counts"]["mt_hits"] > 0 and exp["counts"]["clause_rejected"] == 0 and exp["counts"]["pixels_changed"] == 0
    assert set(np.unique(got["geometry_ids"])) == {0, 1, U.INVALID}
    assert st["pair_tests"] < st["n_rays"] * st["n_triangles"]      # (every pair tested would be no hierarchy at all)
