"""m3d_voxel_down_sample / _multi on the MI355X: the output points, normals and colours equal the plain-C restatement of the
contract (tests/cpp/voxel_ref.c) BIT FOR BIT and in the same order -- every comparison is np.array_equal on the fp64
arrays viewed as uint64 -- over sizes 1 .. 250 000 x six cloud shapes x three voxel sizes, with normals, NaN normals,
colours and neither; points on voxel faces; skew; wide keys and the forced general path; the seams of the kernels (0 .. 3 sort passes at exact voxel counts, 63 .. 129
members around the 64-member batch of the means with NaN normals on its edges, element counts around the sort's, the scan's
and the bounds kernel's tiles); the golden PLY; the multi-level
call; the trace; 1 M points, repeated and from four threads; the errors; the Python API, the C++ mirror, and the chain
into preprocess_fragment."""
import os
import subprocess
import threading

import numpy as np
import pytest

from fps_ref_util import shaped_clouds
from voxel_ref_util import (SEAM_HEAD, VOXEL_ELEMENT_SEAMS, VOXEL_PASS_SEAMS, bits, build_ref, extent, faces_cloud,
                            faces_fraction_moved, same, seam_head, seam_normals, unit_normals, voxel_seam_cloud)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("voxel_ref"))


@pytest.fixture(scope="module")
def dev(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device")
    return capi


def _same_all(got, exp):
    return (same(got, exp) and np.array_equal(got["first_index"], exp["first_index"])
            and np.array_equal(got["point_to_voxel"], exp["point_to_voxel"]))


def _variants(n, seed):
    """(name, normals, colours): with normals, with normals containing NaN rows, with colours (and normals), with neither"""
    rng = np.random.default_rng(seed)
    col = rng.uniform(0, 1, (n, 3))
    return [("neither", None, None), ("normals", unit_normals(n, seed), None),
            ("nan_normals", unit_normals(n, seed, max(n // 20, 1)), None), ("colours", unit_normals(n, seed + 1), col),
            ("colours_only", None, col)]


@pytest.mark.parametrize("n", [1, 2, 3, 513, 5841])
def test_shapes_sizes_attributes(dev, ref, n):
    for name, pts in shaped_clouds(n, 11).items():
        for div in (3, 50, 2000):
            v = extent(pts) / div
            for vname, nrm, col in _variants(n, div):
                got = dev.voxel_down_sample(pts, v, nrm, col, trace=True)
                assert _same_all(got, ref(pts, v, nrm, col)), (name, n, div, vname)


def test_shapes_250k(dev, ref):
    """every shape x voxel size without attributes, and the attribute variants dealt round over the 18 combinations"""
    n = 250_000
    variants = _variants(n, 5)
    k = 0
    for name, pts in shaped_clouds(n, 4).items():
        for div in (3, 50, 2000):
            v = extent(pts) / div
            for vname, nrm, col in (variants[0], variants[1 + k % 4]):
                got = dev.voxel_down_sample(pts, v, nrm, col, trace=True)
                assert _same_all(got, ref(pts, v, nrm, col)), (name, div, vname)
            k += 1


@pytest.mark.parametrize("v", [0.01, 0.005, 0.02, 0.0137, 0.003])
def test_points_on_voxel_faces(dev, ref, v):
    """a reciprocal instead of the division would move these points to a neighbouring voxel"""
    pts = faces_cloud(200_000, v, seed=3)
    assert faces_fraction_moved(pts, v) >= 0.05      # (numpy alone: the case is not vacuous)
    assert _same_all(dev.voxel_down_sample(pts, v, trace=True), ref(pts, v))


def test_skew(dev, ref):
    rng = np.random.default_rng(21)
    big = rng.uniform(-1, 1, (1_000_000, 3))
    nrm = unit_normals(len(big), 3, 1000)
    got, st = dev.voxel_down_sample(big, 10.0, nrm, trace=True, stats=True)      # all points in one voxel
    assert len(got["points"]) == 1 and st["sort_passes"] == 0
    assert _same_all(got, ref(big, 10.0, nrm))
    half = big.copy()
    half[::2] = half[0] + 1e-4 * rng.uniform(0, 1, (500_000, 3))                # half the points in one voxel, the rest spread
    assert _same_all(dev.voxel_down_sample(half, 0.01, trace=True), ref(half, 0.01))
    dup = rng.uniform(-1, 1, (300, 3))[rng.integers(0, 300, 50_000)]            # exact duplicates
    for v in (0.05, 1e-9 * 4):
        assert _same_all(dev.voxel_down_sample(dup, v, trace=True), ref(dup, v)), v
    z = rng.choice([0.0, -0.0, 1.0, -1.0], (20_000, 3))                         # signed zeros
    zn = rng.choice([0.0, -0.0], (20_000, 3))
    for v in (0.5, 1.0, 7.0):
        assert _same_all(dev.voxel_down_sample(z, v, zn, zn, trace=True), ref(z, v, zn, zn)), v


def test_wide_keys_and_forced_general_path(dev, ref):
    rng = np.random.default_rng(22)
    w = rng.uniform(0, 1e9, (60_000, 3))                                          # 1e9 voxels per axis: 90 key bits
    w[:20_000] = w[20_000:40_000] + rng.uniform(0, 0.4, (20_000, 3))              # ... with shared voxels
    got, st = dev.voxel_down_sample(w, 1.0, trace=True, stats=True)
    assert st["path"] == dev.VOXEL_PATH_WIDE
    exp = ref(w, 1.0)
    assert _same_all(got, exp) and len(exp["points"]) < len(w)
    pts = shaped_clouds(65_537, 6)["clusters"]
    nrm = unit_normals(len(pts), 6, 500)
    v = extent(pts) / 60
    fast, st_fast = dev.voxel_down_sample(pts, v, nrm, trace=True, stats=True)
    dev.voxel_force_path(dev.VOXEL_PATH_WIDE)
    try:
        wide, st_wide = dev.voxel_down_sample(pts, v, nrm, trace=True, stats=True)
    finally:
        dev.voxel_force_path(0)
    assert st_fast["path"] == dev.VOXEL_PATH_PACKED and st_wide["path"] == dev.VOXEL_PATH_WIDE
    assert _same_all(wide, fast) and _same_all(fast, ref(pts, v, nrm))


# ---- the kernels' seams (the clouds and what they promise: voxel_ref_util.py, shown on the CPU in test_voxel.py): every
# result equals the checker's bit for bit, trace included
def _seam_run(dev, ref, pts, nrm, col, wide, passes):
    dev.voxel_force_path(dev.VOXEL_PATH_WIDE if wide else 0)
    try:
        got, st = dev.voxel_down_sample(pts, 1.0, nrm, col, trace=True, stats=True)
    finally:
        dev.voxel_force_path(0)
    exp = ref(pts, 1.0, nrm, col)
    assert st["path"] == (dev.VOXEL_PATH_WIDE if wide else dev.VOXEL_PATH_PACKED)
    assert st["sort_passes"] == passes and st["n_voxels"] == len(exp["points"])
    assert _same_all(got, exp)
    return exp


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("m,n,head,passes", VOXEL_PASS_SEAMS)
def test_sort_pass_seams(dev, ref, m, n, head, passes, wide):
    """m voxels exactly, on both sides of every change of the number of 8-bit sort passes: 0, 1, 1, 2, 2, 3"""
    pts, cell = voxel_seam_cloud(m, n, head, seed=m)
    exp = _seam_run(dev, ref, pts, seam_normals(cell, m), None, wide, passes)
    assert len(exp["points"]) == m


@pytest.mark.parametrize("colours", [False, True])
def test_member_seams(dev, ref, colours):
    """voxels of 1, 63, 64, 65, 128 and 129 members around the 64 voxel_means_k stages at a time, NaN normals on the last
    member of a batch and the first of the next: a skip flag that outlived its batch would drop or add a normal"""
    pts, cell = voxel_seam_cloud(257, 4096, SEAM_HEAD, seed=257)
    col = np.random.default_rng(257).uniform(0, 1, pts.shape) if colours else None
    exp = _seam_run(dev, ref, pts, seam_normals(cell, 257), col, False, 2)
    assert all(int((exp["counts"] == h).sum()) == 1 for h in SEAM_HEAD[1:])


@pytest.mark.parametrize("nan_normals", [False, True])
@pytest.mark.parametrize("n", VOXEL_ELEMENT_SEAMS)
def test_element_seams(dev, ref, n, nan_normals):
    """n around the sort's round and tile, the scan's tile, the bounds kernel's grid and the 256 tile sums of the scan's
    middle step.  Without attributes: the highest cell's only point is the last row.  With NaN-row normals: the same
    cloud reversed, so that the lattice corner -- which alone sets vmin -- is the last row"""
    m = min(n, 300)
    pts, _ = voxel_seam_cloud(m, n, seam_head(m, n), seed=n, highest_last=True)
    nrm = None
    if nan_normals:
        pts = np.ascontiguousarray(pts[::-1])
        nrm = unit_normals(n, n, max(n // 20, 1))
    exp = _seam_run(dev, ref, pts, nrm, None, False, ((m - 1).bit_length() + 7) // 8)
    assert len(exp["points"]) == m


def test_golden_ply(dev, ref):
    """the examples' cloud at the examples' sizes.  The fixture stores points only; its normals are the ones the examples
    would down-sample with it: estimated from the cloud (hybrid search, 0.02 / 30), then carried through the voxels"""
    from misc3d_amd import io
    d = io.read_ply(os.path.join(ROOT, "tests", "golden", "segmentation_test.ply"))
    pts = np.ascontiguousarray(d["points"])
    assert len(pts) == 40458
    nrm = d["normals"] if d["normals"] is not None else dev.estimate_normals(pts, radius=0.02, max_nn=30)
    assert nrm.shape == pts.shape
    for v in (0.01, 0.005):
        assert _same_all(dev.voxel_down_sample(pts, v, nrm, d["colors"], trace=True), ref(pts, v, nrm, d["colors"])), v
        assert _same_all(dev.voxel_down_sample(pts, v, trace=True), ref(pts, v)), v


def test_multi_level_and_trace(dev, ref):
    pts = shaped_clouds(100_000, 8)["sphere"]
    nrm = unit_normals(len(pts), 8, 100)
    col = np.random.default_rng(8).uniform(0, 1, pts.shape)
    v = extent(pts) / 40
    sizes = [v, v / 2, v / 4]
    levels = dev.voxel_down_sample_multi(pts, sizes, nrm, col, trace=True)
    assert len(levels) == 3
    for level, s in zip(levels, sizes):
        single = dev.voxel_down_sample(pts, s, nrm, col, trace=True)
        assert _same_all(level, single) and _same_all(level, ref(pts, s, nrm, col)), s
        # the trace is consistent with the outputs: the means recomputed on the host from point_to_voxel, in index order
        p2v, first = level["point_to_voxel"].astype(np.int64), level["first_index"].astype(np.int64)
        m = len(first)
        assert np.all(np.diff(first) > 0) and np.array_equal(p2v[first], np.arange(m))
        seen_first = np.full(m, len(pts), dtype=np.int64)
        np.minimum.at(seen_first, p2v, np.arange(len(pts)))
        assert np.array_equal(seen_first, first)
        order = np.argsort(p2v, kind="stable")
        starts = np.searchsorted(p2v[order], np.arange(m))
        counts = np.diff(np.append(starts, len(pts)))
        sums = np.zeros((m, 3))
        for k in range(int(counts.max())):                     # the k-th member of every voxel that has one
            rows = np.nonzero(counts > k)[0]
            sums[rows] += pts[order[starts[rows] + k]]
        assert np.array_equal(bits(sums / counts[:, None].astype(np.float64)), bits(level["points"]))


def test_1m_repeatable_and_threads(dev, ref):
    big = np.random.default_rng(23).uniform(-1, 1, (1_000_000, 3))
    v = 2.0 / 200
    first = dev.voxel_down_sample(big, v, trace=True)
    assert _same_all(first, ref(big, v))
    assert _same_all(dev.voxel_down_sample(big, v, trace=True), first)
    out = [None] * 4

    def work(k):
        out[k] = dev.voxel_down_sample(big, v, trace=True)
    ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for k in range(4):
        assert out[k] is not None and _same_all(out[k], first), k


def test_errors(dev):
    pts = np.random.default_rng(24).uniform(-1, 1, (5000, 3))
    bad = pts.copy()
    bad[4321, 2] = np.nan
    bad[77, 0] = -np.inf
    with pytest.raises(dev.M3DError) as e:
        dev.voxel_down_sample(bad, 0.1)
    assert e.value.code == dev.ERR_NON_FINITE and "point 77 " in str(e.value)
    for v in (0.0, -0.1, float("nan")):
        with pytest.raises(dev.M3DError) as e:
            dev.voxel_down_sample(pts, v)
        assert e.value.code == dev.ERR_INVALID_ARG and "[VoxelDownSample] voxel_size <= 0." in str(e.value)
    with pytest.raises(dev.M3DError) as e:
        dev.voxel_down_sample(pts, 1e-12)
    assert e.value.code == dev.ERR_INVALID_ARG and "[VoxelDownSample] voxel_size is too small." in str(e.value)
    with pytest.raises(dev.M3DError) as e:
        dev.voxel_down_sample_multi(pts, [0.1, 1e-12])
    assert "voxel_size is too small." in str(e.value)
    # the largest size the too-small test lets through still works (31-bit indices)
    span = float((pts.max(axis=0) - pts.min(axis=0)).max())
    tiny = span / 2.0e9
    got = dev.voxel_down_sample(pts[:300], tiny, trace=True)
    assert len(got["points"]) == 300 and np.array_equal(bits(got["points"]), bits(pts[:300]))


def test_python_api(dev, ref):
    import misc3d_amd as m3d
    pts = shaped_clouds(5841, 1)["sphere"]
    nrm = unit_normals(len(pts), 1)
    col = np.random.default_rng(1).uniform(0, 1, pts.shape)
    v = extent(pts) / 30
    exp = ref(pts, v, nrm, col)

    class Obj:
        points, normals, colors = pts, nrm, col
    p, n_, c = m3d.preprocessing.voxel_down_sample(Obj(), v)
    assert same({"points": p, "normals": n_, "colors": c}, exp)
    p, n_, c, first, p2v = m3d.preprocessing.voxel_down_sample(pts, v, colors=col, trace=True)
    assert n_ is None and np.array_equal(bits(p), bits(exp["points"])) and np.array_equal(bits(c), bits(exp["colors"]))
    assert first.dtype == np.int64 and np.array_equal(first, exp["first_index"].astype(np.int64))
    assert p2v.shape == (len(pts),) and np.array_equal(p2v, exp["point_to_voxel"].astype(np.int64))
    levels = m3d.preprocessing.voxel_down_sample_multi(pts, [v, v / 2, v / 4], nrm)
    for level, s in zip(levels, (v, v / 2, v / 4)):
        assert same({"points": level[0], "normals": level[1], "colors": level[2]}, ref(pts, s, nrm))
    with pytest.raises(RuntimeError, match="voxel_size is too small"):
        m3d.preprocessing.voxel_down_sample(pts, 1e-13)


def test_cpp_mirror(dev, ref, tmp_path):
    exe = str(tmp_path / "voxel_mirror")
    lib = os.path.join(ROOT, "misc3d_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_voxel_mirror.cpp"), "-o", exe, "-L", lib, "-lmisc3d_amd",
                    "-lpthread", "-Wl,-rpath," + lib], check=True)
    pts = shaped_clouds(3000, 6)["clusters"]
    nrm = unit_normals(len(pts), 6, 50)
    col = np.random.default_rng(6).uniform(0, 1, pts.shape)
    v = extent(pts) / 25
    for flags in (3, 0):
        blob = tmp_path / f"cloud{flags}.bin"
        blob.write_bytes(np.array([len(pts), flags], dtype=np.uint64).tobytes() + pts.tobytes()
                         + (nrm.tobytes() + col.tobytes() if flags else b""))
        r = subprocess.run([exe, str(blob), repr(v)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.split("\n")
        at = 0
        for tag, s in (("single", v), ("level", v), ("level", v / 2), ("level", v / 4)):
            exp = ref(pts, s, nrm if flags else None, col if flags else None)
            m = len(exp["points"])
            assert lines[at] == f"{tag} {m} {int(bool(flags))} {int(bool(flags))}"
            rows = np.array([[int(t, 16) for t in ln.split()] for ln in lines[at + 1: at + 1 + m]], dtype=np.uint64)
            cols = [exp["points"]] + ([exp["normals"], exp["colors"]] if flags else [])
            assert np.array_equal(rows, np.hstack([bits(a) for a in cols])), (tag, s)
            at += 1 + m
        assert lines[at] == f"select 2 {int(bool(flags))} {int(bool(flags))}"
        at += 1
        if flags:
            assert lines[at] == "1"
            at += 1
        assert lines[at] == "empty 0"
        assert lines[at + 1] == "[Misc3D Error] [VoxelDownSample] voxel_size <= 0."


def test_chain_into_preprocess_fragment(dev, ref):
    """the documented order is what makes downstream results reproducible: the device's down-sampled cloud and the
    checker's give the same normals and FPFH descriptors, row for row"""
    pts = shaped_clouds(60_000, 9)["sphere"]
    v = extent(pts) / 60
    got = dev.voxel_down_sample(pts, v)["points"]
    exp = ref(pts, v)["points"]
    assert np.array_equal(bits(got), bits(exp))
    n_got, f_got = dev.preprocess_fragment(got, v)
    n_exp, f_exp = dev.preprocess_fragment(exp, v)
    assert np.array_equal(bits(n_got), bits(n_exp)) and np.array_equal(bits(f_got), bits(f_exp))
    assert np.isfinite(f_got).all() and f_got.shape == (len(got), 33)
