"""misc3d.preprocessing.farthest_point_sampling on the MI355X: bit-exact against the plain-C restatement of the reference's
loop (tests/cpp/fps_ref.c) on every device path -- one workgroup (M3D_FPS_PATH_SINGLE), the tile-pruned steps
(M3D_FPS_PATH_PRUNED) and the same steps with no tile skipped (M3D_FPS_PATH_DENSE, forced through the measurement hook) --
over sizes 1 .. 250 000, six cloud shapes and the quirk clouds; pruned == dense at 1 M x 10 000; repeatability, four threads
on one device, the python API and the C++ mirror header."""
import os
import subprocess
import threading

import numpy as np
import pytest

from fps_ref_util import build_ref, quirk_clouds, shaped_clouds

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
