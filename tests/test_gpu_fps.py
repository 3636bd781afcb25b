"""misc3d.preprocessing.farthest_point_sampling on the MI355X: bit-exact against the plain-C restatement of the reference's
loop (tests/cpp/fps_ref.c) on every device path -- one workgroup (M3D_FPS_PATH_SINGLE), the tile-pruned steps
(M3D_FPS_PATH_PRUNED) and the same steps with no tile skipped (M3D_FPS_PATH_DENSE, forced through the measurement hook) --
over sizes 1 .. 250 000, six cloud shapes and the quirk clouds; every size at which a kernel changes its form, with its
neighbours (the four one-workgroup instantiations, the crossover, full tiles, the tile loop's second trip at 3.1 M points,
the unsorted layout); pruned == dense at 1 M x 10 000; repeatability, four threads on one device, the python API and the C++
mirror header."""
import os
import subprocess
import threading

import numpy as np
import pytest

from fps_ref_util import (FPS_CROSSOVER, FPS_SECOND_TRIP_N, FPS_SINGLE_SEAMS, FPS_TILE, build_ref, fps_seam_cloud,
                          fps_tile_edge_cloud, fps_unsorted_clouds, quirk_clouds, shaped_clouds)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("fps_ref"))


@pytest.fixture(scope="module")
def dev(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device")
    return capi


def _run(capi, pts, S, path=0):
    capi.fps_force_path(path)
    try:
        return capi.farthest_point_sampling(pts, S, stats=True)
    finally:
        capi.fps_force_path(0)


def _paths(n):
    return ([1] if n <= 8192 else []) + [2, 3]


def test_tiny_and_small_sizes(dev, ref):
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 513):
        pts = rng.uniform(-1, 1, (n, 3))
        for S in sorted({1, 2, n - 1} & set(range(1, n + 1))):
            exp = ref(pts, S)
            for path in _paths(n):
                got, st = _run(dev, pts, S, path)
                assert np.array_equal(got, exp), (n, S, path)
                assert st["path"] == (path if S < n else 0)


@pytest.mark.parametrize("n", [513, 5841])
def test_shapes_every_path(dev, ref, n):
    for name, pts in shaped_clouds(n, 11).items():
        S = min(1000, n - 1)
        exp = ref(pts, S)
        for path in _paths(n):
            got, _ = _run(dev, pts, S, path)
            assert np.array_equal(got, exp), (name, n, path)


def test_quirk_clouds_every_path(dev, ref):
    for name, pts in quirk_clouds(2).items():
        for S in (1, 2, 60, len(pts) - 1):
            exp = ref(pts, S)
            for path in _paths(len(pts)):
                got, _ = _run(dev, pts, S, path)
                assert np.array_equal(got, exp), (name, S, path)


def test_quirks_on_the_pruned_path_at_scale(dev, ref):
    """the quirk rows inside a cloud large enough for the tiles: non-finite rows left out of the tiles as constant
    +inf candidates, overflowing squares, duplicates and signed zeros among sorted tiles"""
    rng = np.random.default_rng(9)
    pts = rng.uniform(-1, 1, (20000, 3))
    pts[5000:5100] = pts[0]
    pts[7000:7050] = -0.0
    big = rng.uniform(-1, 1, (20000, 3)) * 1e155
    nan_mid = pts.copy()
    nan_mid[1234, 1] = np.nan
    nan_mid[4321] = np.inf
    for name, p in (("dups_zeros", pts), ("overflow", big), ("nonfinite", nan_mid)):
        exp = ref(p, 300)
        for path in (2, 3):
            got, _ = _run(dev, p, 300, path)
            assert np.array_equal(got, exp), (name, path)


# ---- the kernels' seams: every size at which a kernel takes another form, one below and one above (the clouds and what they
# promise: fps_ref_util.py, shown on the CPU in test_preprocessing.py).  Every result is bit-equal to the restatement.
@pytest.fixture(scope="module")
def expected(ref):
    """the restatement's result for a named cloud, computed once and shared by the paths"""
    cache = {}

    def get(key, pts, S):
        if (key, S) not in cache:
            r = ref(pts, S)
            r.setflags(write=False)
            cache[(key, S)] = r
        return cache[(key, S)]
    return get


def _tiles(n):
    return max(1, -(-n // FPS_TILE))


def _check(dev, expected, key, pts, S, path, n_tiles=None):
    got, st = _run(dev, pts, S, path)
    assert np.array_equal(got, expected(key, pts, S)), (key, S, path)
    assert st["path"] == (path or (1 if len(pts) <= 8192 else 2))
    if st["path"] != 1:
        assert st["tile_steps"] == (n_tiles or _tiles(len(pts))) * (S - 1)
        if path == 3:
            assert st["tiles_updated"] == st["tile_steps"]
    return st


@pytest.mark.parametrize("path", [1, 2, 3])
@pytest.mark.parametrize("n", FPS_SINGLE_SEAMS)
def test_single_instantiation_seams(dev, expected, n, path):
    """fps_single_k<1, 2, 4, 8> at 1024, 2048, 4096, 8192 points, one below and one above: the two far points sit at the end
    of the input, in the highest slot in use; at 8192 no padding slot is left.  The tile paths at the same sizes"""
    _check(dev, expected, ("seam", n), fps_seam_cloud(n, n), 64, path)


@pytest.mark.parametrize("path", [1, 2, 3])
@pytest.mark.parametrize("n", [1025, 8192])
@pytest.mark.parametrize("S", [2, 3, -1])
def test_single_sample_counts(dev, expected, S, n, path):
    """one and two steps (each parity of the double-buffered LDS alone) and all n - 1 samples in one launch"""
    _check(dev, expected, ("seam", n), fps_seam_cloud(n, n), S if S > 0 else n - 1, path)


@pytest.mark.parametrize("path", [1, 2, 3])
@pytest.mark.parametrize("n", [2049, 4097])
def test_ties_across_slots(dev, expected, n, path):
    """exact distance ties on a lattice: the lowest index wins across register slots, lanes, waves and tiles"""
    _check(dev, expected, ("lattice", n), shaped_clouds(n)["lattice"], 500, path)


@pytest.mark.parametrize("S,path", [(64, 0), (8192, 0), (64, 3), (8192, 3)])
def test_crossover_8193(dev, expected, S, path):
    """one point past the one-workgroup path: 17 tiles, the last one holds a single point -- one of the first three samples"""
    n = FPS_CROSSOVER
    st = _check(dev, expected, ("seam", n), fps_seam_cloud(n, n), S, path, n_tiles=17)
    assert st["path"] == (path or 2)


def test_crossover_both_sides(dev, expected):
    """8192 points still take the one-workgroup path by default; 8193 cannot be forced onto it"""
    st = _check(dev, expected, ("seam", 8192), fps_seam_cloud(8192, 8192), 64, 0)
    assert st["path"] == 1
    with pytest.raises(dev.M3DError, match="at most 8192 points"):
        _run(dev, fps_seam_cloud(FPS_CROSSOVER, 0), 64, 1)


@pytest.mark.parametrize("path", [2, 3])
@pytest.mark.parametrize("nonfinite", [0, 3])
@pytest.mark.parametrize("n_finite", [20 * FPS_TILE, 20 * FPS_TILE + 1])
def test_tile_edges(dev, expected, n_finite, nonfinite, path):
    """the finite points fill 20 tiles to the last slot, or leave one point for a 21st; with three non-finite rows outside
    the tiles (the constant +inf candidate) and with none"""
    pts = fps_tile_edge_cloud(n_finite, nonfinite, 3)
    _check(dev, expected, ("edge", n_finite, nonfinite), pts, 64, path, n_tiles=_tiles(n_finite))


@pytest.fixture(scope="module")
def second_trip_cloud():
    pts = np.random.default_rng(31).uniform(-1, 1, (FPS_SECOND_TRIP_N, 3))
    pts.setflags(write=False)
    return pts


@pytest.mark.parametrize("path", [0, 3])
def test_second_trip_of_the_tile_loop(dev, expected, second_trip_cloud, path):
    """6145 tiles: the step kernel's 1024 workgroups of 4 waves walk them in two trips, a third of the tiles in the second.
    Were that trip lost, all 31 selections would have to fall into the first two thirds: (2/3)^31 ~ 3e-6"""
    S = 32
    st = _check(dev, expected, "second_trip", second_trip_cloud, S, path)
    assert st["path"] == (path or 2) and st["tile_steps"] // (S - 1) > 4096


@pytest.mark.parametrize("path", [0, 3])
@pytest.mark.parametrize("name", ["inf_extent", "inf_extent_nonfinite", "subnormal_extent"])
def test_unsorted_layout(dev, expected, name, path):
    """an extent that overflows or is subnormal: every point in input order in the tiles, the non-finite rows among them and
    no constant candidate"""
    st = _check(dev, expected, ("unsorted", name), fps_unsorted_clouds()[name], 40, path, n_tiles=18)
    assert st["path"] == (path or 2)


def test_65537_default_path(dev, ref):
    clouds = shaped_clouds(65537, 3)
    for name in ("cube", "lattice", "clusters"):
        pts = clouds[name]
        for S in (1000, 4000):
            exp = ref(pts, S)
            got, st = _run(dev, pts, S)
            assert st["path"] == 2 and st["tile_steps"] > 0
            assert np.array_equal(got, exp), (name, S)
    got, _ = _run(dev, clouds["plane"], 1000, 3)
    assert np.array_equal(got, ref(clouds["plane"], 1000))


def test_250k_against_restatement(dev, ref):
    pts = shaped_clouds(250000, 4)["cube"]
    exp = ref(pts, 4000)
    got, st = _run(dev, pts, 4000)
    assert np.array_equal(got, exp)
    assert st["tiles_updated"] < st["tile_steps"]


def test_1m_pruned_equals_dense(dev):
    pts = np.random.default_rng(8).uniform(-1, 1, (1_000_000, 3))
    a, sa = _run(dev, pts, 10000, 2)
    b, sb = _run(dev, pts, 10000, 3)
    assert np.array_equal(a, b)
    assert sa["path"] == 2 and sb["path"] == 3 and sb["tiles_updated"] == sb["tile_steps"]
    assert sa["tiles_updated"] < sa["tile_steps"] // 2
    assert len(np.unique(a)) == 10000


def test_repeatable_and_threads(dev, ref):
    rng = np.random.default_rng(12)
    clouds = [rng.uniform(-1, 1, (n, 3)) for n in (3000, 20000, 3000, 20000)]
    serial = [dev.farthest_point_sampling(p, 500) for p in clouds]
    assert np.array_equal(serial[1], dev.farthest_point_sampling(clouds[1], 500))
    assert np.array_equal(serial[0], ref(clouds[0], 500))
    out = [None] * 4

    def work(k):
        out[k] = [dev.farthest_point_sampling(clouds[k], 500) for _ in range(3)]
    ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for k in range(4):
        for r in out[k]:
            assert np.array_equal(r, serial[k]), k


def test_python_api(dev, ref):
    import misc3d_amd as m3d
    pts = shaped_clouds(5841, 1)["sphere"]
    exp = ref(pts, 1000)

    class Obj:
        points = pts
    lst = m3d.preprocessing.farthest_point_sampling(Obj(), 1000)
    assert isinstance(lst, list) and lst == [int(i) for i in exp]
    arr = m3d.preprocessing.farthest_point_sampling(pts, 1000, as_arrays=True)
    assert arr.dtype == np.int64 and np.array_equal(arr, exp.astype(np.int64))


CPP = r"""
#include <cstdio>
#include <vector>
#include <misc3d/preprocessing/filter.h>
int main(int argc, char** argv) {
    std::FILE* f = std::fopen(argv[1], "rb");
    size_t n = 0;
    if (std::fread(&n, sizeof(n), 1, f) != 1) return 2;
    misc3d::PointCloud pc;
    pc.points_.resize(n);
    if (std::fread(pc.points_.data(), 24, n, f) != n) return 2;
    std::fclose(f);
    misc3d::SetVerbosityLevel(misc3d::VerbosityLevel::Error);
    const std::vector<size_t> idx = misc3d::preprocessing::FarthestPointSampling(pc, 700);
    for (size_t i : idx) std::printf("%zu\n", i);
    const misc3d::PointCloud roi = misc3d::preprocessing::CropROIPointCloud(pc, std::make_tuple(1, 2, 5, 4), std::make_tuple(100, (int)n / 100));
    std::printf("roi %zu\n", roi.points_.size());
    try {
        misc3d::preprocessing::FarthestPointSampling(pc, (int)n + 1);
    } catch (const std::runtime_error& e) {
        std::printf("%s\n", e.what());
    }
    return 0;
}
"""


def test_cpp_mirror(dev, ref, tmp_path):
    src = tmp_path / "fps_mirror.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "fps_mirror")
    lib = os.path.join(ROOT, "misc3d_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", lib,
                    "-lmisc3d_amd", "-lpthread", "-Wl,-rpath," + lib], check=True)
    pts = shaped_clouds(3000, 6)["clusters"]
    blob = tmp_path / "pts.bin"
    blob.write_bytes(np.array([len(pts)], dtype=np.uint64).tobytes() + np.ascontiguousarray(pts).tobytes())
    r = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert np.array_equal(np.array([int(v) for v in lines[:700]], dtype=np.uint64), ref(pts, 700))
    assert lines[700] == "roi %d" % (5 * 3)
    assert lines[701] == "[Misc3D Error] Illegal number of samples: 3001, must <= point size: 3000"
