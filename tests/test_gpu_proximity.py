"""misc3d.segmentation.ProximityExtractor on the MI355X: every case equals the plain-C restatement of the reference's serial
Segment (tests/cpp/proximity_ref.c) exactly -- clusters, their order and the labels -- on the golden cloud, shaped clouds
with analytic normals, a lattice with spacing == radius and the quirk clouds; the nn_indices overload and its errors; a
python evaluator; get_cluster_index_map reuse; 1 M points against the scipy partition; repeatability; four threads on one
device; the C++ mirror header."""
import os
import subprocess
import threading

import numpy as np
import pytest

from proximity_ref_util import build_ref, golden_ply, pca_normals, scipy_partition, voxel_average

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("prox_ref"))


@pytest.fixture(scope="module")
def dev(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device")
    return capi


def _gpu(capi, xyz, radius, kind, dist=0.0, angle=0.0, normals=None, min_size=1, max_size=2**64 - 1):
    off, idx, lab = capi.proximity_segment(xyz, radius, kind, dist, angle, normals, min_size, max_size)
    return [idx[off[c]:off[c + 1]].astype(np.int64).tolist() for c in range(len(off) - 1)], lab.astype(np.int64)


def _same(capi, ref, xyz, radius, kind, **kw):
    exp = ref.segment(xyz, radius, kind, **kw)
    got = _gpu(capi, xyz, radius, kind, **kw)
    assert got[0] == exp[0]
    assert np.array_equal(got[1], exp[1])
    return got


@pytest.fixture(scope="module")
def golden():
    return golden_ply()


@pytest.fixture(scope="module")
def down(golden):
    pts = voxel_average(golden, 0.01)
    return pts, pca_normals(pts, 0.02)


def test_golden_distance(dev, ref, golden):
    cl, _ = _same(dev, ref, golden, 0.01, "distance", dist=0.01)
    assert len(cl) > 1


@pytest.mark.parametrize("ang", [30.0, -30.0])
def test_golden_downsampled_normals(dev, ref, down, ang):
    pts, nrm = down
    _same(dev, ref, pts, 0.02, "distance_normals", dist=0.02, angle=ang, normals=nrm, min_size=100)
    _same(dev, ref, pts, 0.02, "normals", angle=ang, normals=nrm)


def _shapes(seed=3):
    rng = np.random.default_rng(seed)
    out = {}
    b = rng.uniform(-1, 1, (6000, 3))
    ax = rng.integers(0, 3, 6000)
    b[np.arange(6000), ax] = np.sign(b[np.arange(6000), ax])
    nb = np.zeros_like(b)
    nb[np.arange(6000), ax] = b[np.arange(6000), ax]
    out["box"] = (b, nb)
    p = rng.uniform(-1, 1, (5000, 3))
    p[:, 2] = np.where(p[:, 0] > 0, 0.0, 0.3 * p[:, 0])
    npl = np.where(p[:, :1] > 0, [[0, 0, 1.0]], [[-0.3, 0, 1.0]] / np.linalg.norm([-0.3, 0, 1.0]))
    out["planes"] = (p, npl)
    v = rng.standard_normal((5000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    out["sphere"] = (v * 0.8, v)
    return out


@pytest.mark.parametrize("name", ["box", "planes", "sphere"])
def test_shapes_with_analytic_normals(dev, ref, name):
    pts, nrm = _shapes()[name]
    for kind, dist, ang in (("distance", 0.05, 0.0), ("normals", 0.0, 20.0), ("distance_normals", 0.06, 15.0),
                            ("distance_normals", 0.08, -15.0), ("normals", 0.0, 0.0), ("normals", 0.0, -0.0),
                            ("normals", 0.0, 180.0), ("normals", 0.0, 200.0), ("distance_normals", 0.1, float("nan"))):
        _same(dev, ref, pts, 0.08, kind, dist=dist, angle=ang, normals=nrm)


def test_lattice_spacing_equals_radius(dev, ref):
    g = np.stack(np.meshgrid(*[np.arange(14) * 0.05] * 3, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(1)
    g = g[rng.permutation(len(g))]
    g[::5] += 1e-3   # every fifth point pushed past the radius from its neighbours
    for dist in (0.05, np.nextafter(0.05, 1.0), 1.0):
        _same(dev, ref, g, 0.05, "distance", dist=dist)


def test_quirk_clouds(dev, ref):
    rng = np.random.default_rng(4)
    xyz = rng.uniform(0, 1, (4000, 3))
    xyz[rng.integers(0, 4000, 500)] = xyz[rng.integers(0, 4000, 500)]   # duplicates
    xyz[10, 0] = np.nan
    xyz[20] = np.inf
    xyz[30, 2] = -np.inf
    nrm = rng.standard_normal((4000, 3)) * rng.uniform(0.5, 1.5, (4000, 1))   # unnormalised: dots past +-1
    nrm[40] = np.nan
    for kw in (dict(kind="distance", dist=0.04), dict(kind="distance_normals", dist=0.05, angle=60.0, normals=nrm),
               dict(kind="normals", angle=-70.0, normals=nrm)):
        for mn, mx in ((0, 2**64 - 1), (1, 2**64 - 1), (100, 2**64 - 1), (1, 50), (2, 3)):
            _same(dev, ref, xyz, 0.05, min_size=mn, max_size=mx, **kw)
    pairs = np.repeat(rng.uniform(0, 100, (50, 3)), 2, axis=0) + np.array([[0, 0, 0], [0.01, 0, 0]] * 50)
    cl, _ = _same(dev, ref, pairs, 0.02, "distance", dist=0.02)   # fifty equal-sized clusters
    assert [c[0] for c in cl] == sorted(c[0] for c in cl)
    for n in (0, 1):
        _same(dev, ref, np.zeros((n, 3)), 0.1, "distance", dist=0.1)


def test_errors(dev):
    xyz = np.zeros((10, 3))
    with pytest.raises(dev.M3DError, match="Index exceed size of data!"):
        dev.proximity_segment(xyz, 0.1, "normals", 0.0, 30.0, np.zeros((9, 3)))
    with pytest.raises(dev.M3DError):
        dev.proximity_segment(xyz, -1.0, "distance", 0.1)


def test_nn_overload(dev, ref):
    rng = np.random.default_rng(8)
    xyz = rng.uniform(0, 1, (3000, 3))
    nrm = rng.standard_normal((3000, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    from scipy.spatial import cKDTree
    lists = [list(l) for l in cKDTree(xyz).query(xyz, k=8)[1]]
    lists[5] = []
    lists[6] = [6]
    off = np.zeros(3001, np.uint64)
    off[1:] = np.cumsum([len(l) for l in lists])
    ind = np.array([j for l in lists for j in l], np.uint64)
    for kw in (dict(kind="distance", dist=0.03), dict(kind="distance_normals", dist=0.05, angle=45.0, normals=nrm)):
        exp = ref.segment_nn(xyz, lists, **kw)
        o, i, lab = dev.proximity_segment_nn(xyz, off, ind, kw["kind"], kw["dist"], kw.get("angle", 0.0), kw.get("normals"))
        assert [i[o[c]:o[c + 1]].astype(np.int64).tolist() for c in range(len(o) - 1)] == exp[0]
        assert np.array_equal(lab.astype(np.int64), exp[1])
    with pytest.raises(dev.M3DError, match="The number of input data size are not equal!"):
        dev.proximity_segment_nn(xyz, off[:-1], ind, "distance", 0.03)
    bad = ind.copy()
    bad[7] = 3000
    with pytest.raises(dev.M3DError):
        dev.proximity_segment_nn(xyz, off, bad, "distance", 0.03)


def test_python_api_and_subclass(dev, ref, down):
    import misc3d_amd as m3d
    pts, nrm = down
    exp, exp_lab = ref.segment(pts, 0.02, "distance_normals", dist=0.02, angle=30.0, normals=nrm, min_size=100)
    pe = m3d.segmentation.ProximityExtractor(100)
    got = pe.segment(pts, 0.02, m3d.segmentation.DistanceNormalsProximityEvaluator(nrm, 0.02, 30))
    assert got == exp
    assert pe.get_cluster_num() == len(exp)
    assert np.array_equal(np.array(pe.get_cluster_index_map()), exp_lab)
    arr = pe.segment(pts, 0.02, m3d.segmentation.DistanceNormalsProximityEvaluator(nrm, 0.02, 30), as_arrays=True)
    assert [a.tolist() for a in arr] == exp and all(a.dtype == np.int64 for a in arr)

    class MyDistance(m3d.segmentation.BaseProximityEvaluator):
        def __call__(self, i, j, dist):
            return dist < 0.015

    small = pts[:3000]
    exp2, _ = ref.segment(small, 0.02, "distance", dist=0.015)
    assert m3d.segmentation.ProximityExtractor().segment(small, 0.02, MyDistance()) == exp2
    assert m3d.segmentation.ProximityExtractor().segment(small, 0.02, m3d.segmentation.DistanceProximityEvaluator(0.015)) == exp2

    class Overridden(m3d.segmentation.DistanceProximityEvaluator):
        def __call__(self, i, j, dist):
            return False

    assert len(m3d.segmentation.ProximityExtractor().segment(small, 0.02, Overridden(1.0))) == len(small)
    # reuse: the index map keeps the larger cloud's stale entries past the smaller cloud (the reference's resize)
    pe2 = m3d.segmentation.ProximityExtractor()
    pe2.segment(small, 0.02, m3d.segmentation.DistanceProximityEvaluator(0.015))
    first = np.array(pe2.get_cluster_index_map())
    pe2.segment(small[:100], 0.02, m3d.segmentation.DistanceProximityEvaluator(0.015))
    m = np.array(pe2.get_cluster_index_map())
    assert len(m) == 100
    pe2.segment(small, 0.02, m3d.segmentation.DistanceProximityEvaluator(0.015))
    assert np.array_equal(np.array(pe2.get_cluster_index_map()), first)
    with pytest.raises(RuntimeError, match="Index exceed size of data!"):
        pe2.segment(small, 0.02, m3d.segmentation.NormalsProximityEvaluator(nrm[:10], 30))


def test_one_million_points_against_scipy(dev):
    rng = np.random.default_rng(11)
    xyz = rng.uniform(0, 1, (1_000_000, 3))
    off, idx, _ = dev.proximity_segment(xyz, 0.008, "distance", 0.008)
    got = [idx[off[c]:off[c + 1]].astype(np.int64).tolist() for c in range(len(off) - 1)]
    assert got == scipy_partition(xyz, 0.008, dist=0.008)


def test_repeatable_and_threads(dev, down):
    pts, nrm = down
    runs = [dev.proximity_segment(pts, 0.02, "distance_normals", 0.02, 30.0, nrm) for _ in range(5)]
    for r in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(r, runs[0]))
    out, errs = [None] * 4, []

    def work(k):
        try:
            out[k] = dev.proximity_segment(pts, 0.02, "distance_normals", 0.02, 30.0, nrm)
        except Exception as e:   # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs
    for r in out:
        assert all(np.array_equal(a, b) for a, b in zip(r, runs[0]))


def test_radius_neighbors_sorted(dev):
    rng = np.random.default_rng(2)
    xyz = rng.uniform(0, 1, (2000, 3))
    off, idx, d2 = dev.radius_neighbors(xyz, 0.1)
    from scipy.spatial import cKDTree
    exp = cKDTree(xyz).query_ball_point(xyz, 0.1 * 1.0001)
    for i in range(0, 2000, 37):
        row = idx[off[i]:off[i + 1]].astype(np.int64)
        dd = xyz[row] - xyz[i]
        e2 = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
        assert np.array_equal(e2, d2[off[i]:off[i + 1]])
        assert list(zip(e2, row)) == sorted(zip(e2, row))
        want = {j for j in exp[i] if j != i}
        want = {j for j in want if ((xyz[j] - xyz[i])[0] ** 2 + (xyz[j] - xyz[i])[1] ** 2) + (xyz[j] - xyz[i])[2] ** 2 <= 0.01}
        assert set(row.tolist()) == want


CPP = r"""
#include <cstdio>
#include <vector>
#include <misc3d/segmentation/proximity_extraction.h>
int main(int argc, char** argv) {
    std::FILE* f = std::fopen(argv[1], "rb");
    size_t n = 0;
    if (std::fread(&n, sizeof(n), 1, f) != 1) return 2;
    misc3d::PointCloud pc;
    pc.points_.resize(n);
    std::vector<misc3d::Vector3d> normals(n);
    if (std::fread(pc.points_.data(), 24, n, f) != n) return 2;
    if (std::fread(normals.data(), 24, n, f) != n) return 2;
    std::fclose(f);
    misc3d::segmentation::ProximityExtractor pe(10);
    misc3d::segmentation::DistanceNormalsProximityEvaluator ev(normals, 0.02, 30);
    const auto cl = pe.Segment(pc, 0.02, ev);
    std::printf("%zu\n", cl.size());
    for (const auto& c : cl) {
        for (size_t i : c) std::printf("%zu ", i);
        std::printf("\n");
    }
    return 0;
}
"""


def test_cpp_mirror(dev, ref, down, tmp_path):
    src = tmp_path / "prox_mirror.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "prox_mirror")
    lib = os.path.join(ROOT, "misc3d_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", lib,
                    "-lmisc3d_amd", "-lpthread", "-Wl,-rpath," + lib], check=True)
    pts, nrm = down
    blob = tmp_path / "pts.bin"
    blob.write_bytes(np.array([len(pts)], np.uint64).tobytes() + np.ascontiguousarray(pts).tobytes() +
                     np.ascontiguousarray(nrm).tobytes())
    r = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    exp, _ = ref.segment(pts, 0.02, "distance_normals", dist=0.02, angle=30.0, normals=nrm, min_size=10)
    assert int(lines[0]) == len(exp)
    assert [[int(v) for v in l.split()] for l in lines[1:]] == exp
