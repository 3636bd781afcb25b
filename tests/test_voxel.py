"""Voxel down-sampling without a GPU: the plain-C checker (tests/cpp/voxel_ref.c) against an independent numpy restatement of
the contract, its error paths, properties it must have on the clouds the GPU tests use, what the seam clouds of the GPU tests promise (exactly m voxels,
the member counts around the 64-member batch, NaN normals on the batch edges, the bounds set by the last row), and the C ABI's argument checks
and exported symbols."""
import ctypes as C

import numpy as np
import pytest

from fps_ref_util import shaped_clouds
from voxel_ref_util import (SEAM_HEAD, VOXEL_ELEMENT_SEAMS, VOXEL_PASS_SEAMS, RefError, bits, build_ref, extent, faces_cloud,
                            faces_fraction_moved, same, seam_head, seam_normals, unit_normals, voxel_indices, voxel_numpy,
                            voxel_seam_cloud)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("voxel_ref"))


def _same_all(a, b):
    return (same(a, b) and np.array_equal(a["first_index"], b["first_index"])
            and np.array_equal(a["point_to_voxel"], b["point_to_voxel"]) and np.array_equal(a["counts"], b["counts"]))


@pytest.mark.parametrize("n", [1, 2, 3, 513])
def test_checker_equals_numpy_restatement(ref, n):
    rng = np.random.default_rng(n)
    for name, pts in shaped_clouds(n, 11).items():
        for div in (3, 50, 2000):
            v = extent(pts) / div
            nrm = unit_normals(n, 1, 20 if n > 100 else 0)
            col = rng.uniform(0, 1, (n, 3))
            assert _same_all(ref(pts, v, nrm, col), voxel_numpy(pts, v, nrm, col)), (name, n, div)
            assert _same_all(ref(pts, v), voxel_numpy(pts, v)), (name, n, div)


def test_checker_quirks_equal_numpy(ref):
    rng = np.random.default_rng(4)
    z = rng.choice([0.0, -0.0, 1.0, -1.0], (400, 3))                 # signed zeros
    d = rng.uniform(-1, 1, (40, 3))[rng.integers(0, 40, 600)]        # exact duplicates
    f = faces_cloud(800, 0.01)                                       # points on voxel faces
    for name, pts, v in (("zeros", z, 0.5), ("zeros_big", z, 10.0), ("dups", d, 0.1), ("faces", f, 0.01)):
        assert _same_all(ref(pts, v), voxel_numpy(pts, v)), name
    # a normal with a NaN component is left out, the divisor still counts it; -0.0 sums stay +0.0
    pts = np.zeros((3, 3))
    nrm = np.array([[1.0, 0, 0], [np.nan, 1, 1], [0, 0, 1.0]])
    r = ref(pts, 1.0, nrm, -np.zeros((3, 3)))
    assert np.array_equal(r["normals"], [[1 / 3, 0, 1 / 3]]) and np.array_equal(bits(r["colors"]), bits(np.zeros((1, 3))))
    assert _same_all(r, voxel_numpy(pts, 1.0, nrm, -np.zeros((3, 3))))


def test_checker_errors_and_empty(ref):
    pts = np.random.default_rng(0).uniform(-1, 1, (10, 3))
    for v in (0.0, -0.5, float("nan")):
        with pytest.raises(RefError) as e:
            ref(pts, v)
        assert e.value.code == 1 and str(e.value) == "[VoxelDownSample] voxel_size <= 0."
        with pytest.raises(RefError):
            voxel_numpy(pts, v)
    for fn in (ref, voxel_numpy):
        with pytest.raises(RefError) as e:
            fn(pts, 1e-12)
        assert e.value.code == 2 and str(e.value) == "[VoxelDownSample] voxel_size is too small."
    bad = pts.copy()
    bad[7, 1] = np.inf
    with pytest.raises(RefError) as e:
        ref(bad, 0.1)
    assert e.value.code == 3 and e.value.index == 7
    for fn in (ref, voxel_numpy):
        r = fn(np.zeros((0, 3)), 0.1)
        assert r["points"].shape == (0, 3) and len(r["first_index"]) == 0


def test_faces_cloud_moves_under_a_reciprocal():
    """the construction the GPU test relies on: a reciprocal instead of the division changes the voxel of > 5 % of the points"""
    for v in (0.01, 0.005, 0.02, 0.0137, 0.003):
        assert faces_fraction_moved(faces_cloud(200_000, v, seed=3), v) >= 0.05, v


@pytest.mark.parametrize("n", [513, 5841])
def test_checker_properties(ref, n):
    clouds = dict(shaped_clouds(n, 11))
    clouds["faces"] = faces_cloud(n, 0.01)
    for name, pts in clouds.items():
        for div in (3, 50, 2000):
            v = 0.01 if name == "faces" else extent(pts) / div
            r = ref(pts, v)
            assert int(r["counts"].sum()) == n
            fi = r["first_index"].astype(np.int64)
            assert np.all(np.diff(fi) > 0) and fi[0] == 0
            assert np.array_equal(r["point_to_voxel"][fi], np.arange(len(fi)))
            # every mean lies in its voxel's closed cell, up to the rounding of the cell's corners and of the mean
            idx, vmin = voxel_indices(pts, v)
            cell = idx[fi]
            lo, hi = vmin + cell * v, vmin + (cell + 1) * v
            slack = 4 * np.finfo(np.float64).eps * (np.abs(pts).max() + abs(vmin).max() + v)
            assert np.all(r["points"] >= lo - slack) and np.all(r["points"] <= hi + slack), (name, div)


def _seam_promise(r, m, head):
    """from the checker's counts alone: exactly m voxels, and exactly one voxel with each member count of the head (of the
    count 1 at least one: where n < 2 m the dealt voxels cannot but hold single points as well)"""
    counts = r["counts"]
    return len(counts) == m and all(int((counts == h).sum()) == 1 if h > 1 else (counts == 1).any() for h in head)


@pytest.mark.parametrize("m,n,head,passes", VOXEL_PASS_SEAMS + ((300, 524_289, SEAM_HEAD, 2),))
def test_seam_cloud_keeps_its_promise(ref, m, n, head, passes):
    """the clouds of the GPU seam tests: m is exact (so the number of sort passes is known), the member counts around the
    64-member batch are there, vmin is exactly 0, and the two restatements agree with the NaN normals in place"""
    assert passes == ((m - 1).bit_length() + 7) // 8
    pts, cell = voxel_seam_cloud(m, n, head, seed=m)
    assert pts.shape == (n, 3) and np.array_equal(pts.min(axis=0), [0.5, 0.5, 0.5]) and np.array_equal(pts[0], [0.5, 0.5, 0.5])
    nrm = seam_normals(cell, m)
    r = ref(pts, 1.0, nrm)
    assert _seam_promise(r, m, head)
    assert np.array_equal(np.sort(r["counts"]), np.sort(np.bincount(cell)))
    assert not np.isnan(r["normals"]).any()                       # a NaN normal is left out, never added
    if n <= 70_001:
        assert _same_all(r, voxel_numpy(pts, 1.0, nrm))


def test_seam_normals_sit_on_the_batch_edges(ref):
    """in the 65- and 129-member voxels the NaN normals are the members 0, 63, 64 (127, 128) in ascending point index, and
    leaving exactly those out is what the checker does"""
    pts, cell = voxel_seam_cloud(257, 4096, SEAM_HEAD, seed=257)
    nrm = seam_normals(cell, 257)
    bad = np.isnan(nrm).any(axis=1)
    assert int(bad.sum()) == 8 and np.allclose(np.linalg.norm(nrm[~bad], axis=1), 1.0)
    counts = np.bincount(cell)
    r = ref(pts, 1.0, nrm)
    for size, positions in ((65, [0, 63, 64]), (129, [0, 63, 64, 127, 128])):
        (c,) = np.nonzero(counts == size)[0]
        members = np.nonzero(cell == c)[0]
        assert np.nonzero(bad[members])[0].tolist() == positions
        keep = members[~bad[members]]
        acc = np.zeros(3)
        for i in keep:
            acc += nrm[i]
        row = int(r["point_to_voxel"][members[0]])
        assert r["counts"][row] == size and np.array_equal(bits(r["normals"][row]), bits(acc / np.float64(size)))
    others = ~np.isin(cell, np.nonzero((counts == 65) | (counts == 129))[0])
    assert not bad[others].any()


@pytest.mark.parametrize("n", VOXEL_ELEMENT_SEAMS)
def test_element_seam_cloud_keeps_its_promise(ref, n):
    """m = min(n, 300) voxels exactly; the highest cell's single point is the last row and alone sets an upper bound; the
    reversed cloud has the lattice corner, which alone sets vmin, as its last row"""
    m = min(n, 300)
    head = seam_head(m, n)
    pts, cell = voxel_seam_cloud(m, n, head, seed=n, highest_last=True)
    assert cell[n - 1] == m - 1 and int((cell == m - 1).sum()) == 1
    assert (pts[n - 1] >= pts.max(axis=0)).sum() >= 1 and (pts[: n - 1].max(axis=0) < pts.max(axis=0)).any()
    r = ref(pts, 1.0)
    assert _seam_promise(r, m, head) and (len(head) == 6) == (n >= 2047)
    back = ref(pts[::-1], 1.0)
    assert np.array_equal(pts[::-1][n - 1], [0.5, 0.5, 0.5]) and (pts[::-1][: n - 1] > 0.5).all()
    assert len(back["counts"]) == m and np.array_equal(np.sort(back["counts"]), np.sort(r["counts"]))
    if n <= 4097:
        assert _same_all(r, voxel_numpy(pts, 1.0)) and _same_all(back, voxel_numpy(pts[::-1], 1.0))


def test_symbols_exported(capi):
    L = capi.lib()
    for name in ("m3d_voxel_down_sample", "m3d_voxel_down_sample_multi", "m3d_bench_voxel_force_path"):
        assert hasattr(L, name), name
    assert C.sizeof(capi.VoxelStats) == 48


def test_argument_validation_needs_no_gpu(capi):
    pts = np.random.default_rng(1).uniform(-1, 1, (10, 3))
    for v in (0.0, -1.0, float("nan")):
        with pytest.raises(capi.M3DError) as e:
            capi.voxel_down_sample(pts, v)
        assert e.value.code == capi.ERR_INVALID_ARG and str(e.value) == "[Misc3D Error] [VoxelDownSample] voxel_size <= 0."
    with pytest.raises(capi.M3DError) as e:
        capi.voxel_down_sample(pts, float("inf"))
    assert e.value.code == capi.ERR_INVALID_ARG
    with pytest.raises(capi.M3DError) as e:
        capi.voxel_down_sample_multi(pts, [0.1, 0.0, 0.05])     # every size is checked before any level runs
    assert "voxel_size <= 0." in str(e.value)
    # an empty cloud is no error and needs no device
    r = capi.voxel_down_sample(np.zeros((0, 3)), 0.1, trace=True)
    assert r["points"].shape == (0, 3) and len(r["first_index"]) == 0 and len(r["point_to_voxel"]) == 0
    assert [len(l["points"]) for l in capi.voxel_down_sample_multi(np.zeros((0, 3)), [0.1, 0.05])] == [0, 0]
    # null pointers
    L = capi.lib()
    m = C.c_size_t(7)
    assert L.m3d_voxel_down_sample(None, None, None, 5, 0.1, 0, None, None, None, None, None,
                                   C.cast(C.byref(m), C.c_void_p), None) == capi.ERR_INVALID_ARG
    assert m.value == 0
    assert L.m3d_voxel_down_sample(capi._p(pts), None, None, 10, 0.1, 0, None, None, None, None, None, None,
                                   None) == capi.ERR_INVALID_ARG
    assert L.m3d_bench_voxel_force_path(3) == capi.ERR_INVALID_ARG and L.m3d_bench_voxel_force_path(0) == capi.OK
    import misc3d_amd as m3d
    with pytest.raises(RuntimeError, match="voxel_size <= 0"):
        m3d.preprocessing.voxel_down_sample(pts, 0.0)
    out = m3d.preprocessing.voxel_down_sample(np.zeros((0, 3)), 0.1, trace=True)
    assert len(out) == 5 and out[0].shape == (0, 3) and out[1] is None and out[2] is None
