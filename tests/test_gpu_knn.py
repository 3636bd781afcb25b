"""KNearestSearch on the MI355X: every case equals the plain-C restatement of the contract (tests/cpp/knn_ref.c) -- indices,
d2 bits, distance bits and hybrid counts -- through the C ABI, the python class and the C++ mirror, on every device path."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

from knn_ref_util import bits, build_ref, lattice

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNNS = (0, 1, 2, 7, 30, 64, 128, 129, 1000)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("knn_ref"))


@pytest.fixture(scope="module")
def dev(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device")
    yield capi
    capi.knn_force_path(0)


def _same(dev, ref, data, queries, knn, search=0, radius=0.0, path=0, index=None):
    """C ABI (forced path) == restatement; returns the stats dict"""
    dev.knn_force_path(path)
    try:
        ix = index or dev.KnnIndex(data)
        i, d, d2, c, st = ix.search(queries, knn, search, radius, stats=True)
    finally:
        dev.knn_force_path(0)
    ri, rd, rd2, rc = ref.search(data, queries, knn, search, radius)
    assert np.array_equal(c, rc), (c, rc)
    assert np.array_equal(i, ri), (path, knn, np.argwhere(i != ri)[:5])
    assert np.array_equal(bits(d2), bits(rd2))
    assert np.array_equal(bits(d), bits(rd))
    return st


def test_dims_and_sizes(dev, ref):
    rng = np.random.default_rng(1)
    for dim, n, m in ((1, 1, 3), (1, 2000, 40), (2, 700, 30), (3, 1, 5), (3, 5000, 100), (4, 3000, 50), (33, 4000, 70),
                      (64, 1500, 20), (100, 900, 9), (1024, 300, 5)):
        data = rng.standard_normal((n, dim))
        q = rng.standard_normal((m, dim))
        for k in (1, 7, 30, 129):
            _same(dev, ref, data, q, k)


def test_knn_values(dev, ref):
    rng = np.random.default_rng(2)
    for dim in (3, 4, 33):
        n = 1500
        data = rng.uniform(-1, 1, (n, dim))
        q = rng.uniform(-1.2, 1.2, (17, dim))
        ix = dev.KnnIndex(data)
        for k in KNNS + (n, n + 5):
            st = _same(dev, ref, data, q, k, index=ix)
            if k == 0:
                assert st["path"] == 0
            elif k <= 128:
                assert st["path"] == (dev.KNN_PATH_GRID if dim == 3 else dev.KNN_PATH_TILE)
            else:
                assert st["path"] == dev.KNN_PATH_SELECT


def test_ties(dev, ref):
    rng = np.random.default_rng(3)
    for dim in (3, 5):
        base = rng.integers(0, 4, (300, dim)).astype(np.float64)
        dup = np.concatenate([base, base[::-1], base[:50]])            # duplicate rows
        lat = lattice(9 if dim == 3 else 3, dim)                         # integer lattice
        eq = np.full((700, dim), 0.25)                                   # all-equal rows
        for data in (dup, lat, eq):
            q = np.concatenate([data[:10], rng.integers(0, 4, (10, dim)) + 0.5, rng.integers(0, 4, (5, dim)) * 1.0])
            for k in (1, 7, 30, 128, 200):
                for path in (0, dev.KNN_PATH_TILE, dev.KNN_PATH_SELECT):
                    _same(dev, ref, data, q, k, path=path)


def test_special_values(dev, ref):
    rng = np.random.default_rng(4)
    for dim in (3, 7):
        data = rng.standard_normal((2000, dim))
        data[5, 0] = np.nan
        data[6, dim - 1] = np.inf
        data[7, 1] = -np.inf
        data[8] = np.inf
        data[9] = 1e160                     # d2 overflows to +inf
        data[10] = -1e160
        data[11:20] = rng.standard_normal((9, dim)) * 1e-310   # subnormals
        data[20] = 5e-324
        q = rng.standard_normal((30, dim))
        q[0, 0] = np.nan
        q[1] = np.inf
        q[2, 1] = -np.inf
        q[3] = 1e160
        q[4] = 0.0
        q[5] = 1e-312
        q[6] = data[11]
        for k in (1, 7, 30, 129, 2000):
            for path in (0, dev.KNN_PATH_TILE, dev.KNN_PATH_SELECT):
                _same(dev, ref, data, q, k, path=path)


def test_dim3_query_placement(dev, ref):
    rng = np.random.default_rng(5)
    data = rng.uniform(0, 1, (20000, 3))
    data[:2000] = np.round(data[:2000] * 8) / 8          # rows on cell faces of several grid classes
    q = np.concatenate([
        data[rng.integers(0, len(data), 40)],           # the data's own points
        rng.uniform(-0.5, 1.5, (40, 3)),                # inside and just outside the box
        rng.uniform(-1e6, 1e6, (10, 3)),                # far away
        np.array([[1e300, -1e300, 0.5], [-1e308, 0.0, 0.0], [0.5, 0.5, 1e-300]]),
        np.round(rng.uniform(0, 1, (20, 3)) * 16) / 16,  # on cell faces
    ])
    for k in (1, 7, 16, 17, 30, 64, 100, 128):
        st = _same(dev, ref, data, q, k)
        assert st["path"] == dev.KNN_PATH_GRID


def test_paths_agree(dev, ref):
    rng = np.random.default_rng(6)
    for dim, n in ((3, 30000), (33, 5000)):
        data = rng.standard_normal((n, dim))
        q = rng.standard_normal((64, dim))
        ix = dev.KnnIndex(data)
        for k in (1, 10, 30, 128):
            paths = (dev.KNN_PATH_GRID, dev.KNN_PATH_TILE, dev.KNN_PATH_SELECT) if dim == 3 else \
                (dev.KNN_PATH_TILE, dev.KNN_PATH_SELECT)
            for path in paths:
                st = _same(dev, ref, data, q, k, path=path, index=ix)
                assert st["path"] == path


def test_hybrid_quirks_capi(dev, ref):
    rng = np.random.default_rng(7)
    for dim in (3, 6):
        data = rng.uniform(0, 1, (3000, dim))
        q = rng.uniform(-0.2, 1.2, (50, dim))
        q[0] = 50.0                                         # nearest neighbour beyond the radius: count -1
        q[1, 0] = np.nan                                    # NaN distances count as inside
        for r in (0.0, 0.05, 0.1, 0.3, 1e9, -1.0, np.nan, np.inf):
            for k in (0, 1, 2, 7, 30, 200):
                _same(dev, ref, data, q, k, search=dev.KNN_SEARCH_HYBRID, radius=r)


def test_python_api(dev, ref):
    import misc3d_amd as m3d
    rng = np.random.default_rng(8)
    data = rng.random((33, 1000))                      # (dim, N), as the reference reads it
    s = m3d.common.KNearestSearch(data)
    q = rng.random(33)
    idx, dist = s.search_knn(q, 5)
    ri, rd, _, _ = ref.search(data.T, q, 5)
    assert idx == ri[0].tolist() and np.array_equal(bits(dist), bits(rd[0]))
    assert isinstance(idx[0], int) and isinstance(dist[0], float)
    # search dispatch: knn / hybrid tuples and param objects, radius -> ([], [])

    class Knn:
        knn = 9

    r = float(s.search_knn(q, 20)[1][10])                # a radius with neighbours inside and outside

    class Hybrid:
        radius, max_nn = r, 40

    class Radius:
        radius = 0.9

    assert s.search(q, ("knn", 9)) == s.search_knn(q, 9) == s.search(q, Knn())
    assert s.search(q, ("hybrid", r, 40)) == s.search_hybrid(q, r, 40) == s.search(q, Hybrid())
    assert s.search(q, ("radius", 0.9)) == ([], []) == s.search(q, Radius())
    ri, rd, _, rc = ref.search(data.T, q, 40, 2, r)
    hi, hd = s.search_hybrid(q, r, 40)
    assert len(hi) == rc[0] == 10 and hi == ri[0, :rc[0]].tolist() and np.array_equal(bits(hd), bits(rd[0, :rc[0]]))
    # the wrap: single raises ValueError (std::length_error), batch reports -1
    with pytest.raises(ValueError):
        s.search_hybrid(q + 100.0, 0.5, 5)
    with pytest.raises(ValueError):
        s.search_hybrid(q, 0.5, 0)
    bi, bd, bc = s.search_hybrid_batch(np.stack([q + 100.0, q]), 0.5, 5)
    assert bc[0] == -1 and (bi[0] == -1).all() and np.isinf(bd[0]).all()
    # single == batch
    qs = rng.random((25, 33))
    bi, bd = s.search_knn_batch(qs, 12)
    for j in range(25):
        si, sd = s.search_knn(qs[j], 12)
        assert si == bi[j].tolist() and np.array_equal(bits(sd), bits(bd[j]))
    bi, bd, bc = s.search_hybrid_batch(qs, r, 12)
    ri, rd, _, rc = ref.search(data.T, qs, 12, 2, r)
    assert np.array_equal(bc, rc) and np.array_equal(bi, ri) and np.array_equal(bits(bd), bits(rd))
    for j in range(25):
        if bc[j] < 0:
            with pytest.raises(ValueError):
                s.search_hybrid(qs[j], r, 12)
        else:
            si, sd = s.search_hybrid(qs[j], r, 12)
            assert si == bi[j, :bc[j]].tolist()
    # early returns and ValueErrors of the batched forms
    assert s.search_knn(q[:5], 3) == ([], []) and s.search_knn(q, -1) == ([], [])
    with pytest.raises(ValueError):
        s.search_knn_batch(qs[:, :5], 3)
    with pytest.raises(ValueError):
        s.search_knn_batch(qs, -1)
    # geometry / feature / set twice
    pts = rng.random((500, 3))

    class Cloud:
        points = pts

    class Mesh:
        vertices = pts

    class Feat:
        data = pts.T.copy()

    for obj in (Cloud(), Mesh(), Feat()):
        g = m3d.common.KNearestSearch(obj, 4)
        gi, gd = g.search_knn(pts[3], 4)
        assert gi[0] == 3 and gd[0] == 0.0
    assert s.set_geometry(Cloud()) and s.search_knn(pts[7], 1)[0] == [7]
    assert not s.set_geometry(object()) and s.search_knn(pts[7], 1)[0] == [7]      # unchanged
    assert s.set_mat_data(data) and s.search_knn(q, 5)[0] == idx
    assert not s.set_mat_data(np.zeros((33, 0))) and s.search_knn(q, 5) == ([], [])


def test_threads(dev, ref):
    rng = np.random.default_rng(9)
    data = rng.standard_normal((20000, 8))
    q = rng.standard_normal((300, 8))
    ix = dev.KnnIndex(data)
    serial = [ix.search(q[j::4], 20)[0] for j in range(4)]
    out = [None] * 4

    def run(j):
        for _ in range(3):
            out[j] = ix.search(q[j::4], 20)[0]

    th = [threading.Thread(target=run, args=(j,)) for j in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for j in range(4):
        assert np.array_equal(out[j], serial[j])


def _free_device_bytes():
    """hipMemGetInfo of device 0 through the HIP runtime the library itself loaded"""
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipSetDevice(0) == 0
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_no_growth(dev, ref):
    import misc3d_amd as m3d
    rng = np.random.default_rng(10)
    data = rng.standard_normal((3, 40000))
    q = rng.standard_normal((100, 3))
    s = m3d.common.KNearestSearch(data)
    first = s.search_knn_batch(q, 30)

    def cycle():
        for _ in range(10):
            s.set_mat_data(data)
            s.set_mat_data(data)
            assert np.array_equal(s.search_knn_batch(q, 30)[0], first[0])
            t = m3d.common.KNearestSearch(data)
            t.search_knn_batch(q, 200)
            del t

    cycle()
    free0 = _free_device_bytes()
    cycle()
    free1 = _free_device_bytes()
    assert free0 - free1 < (64 << 20), (free0, free1)


def test_mutual_pairs_equal_matcher(dev):
    import misc3d_amd as m3d
    from misc3d_amd import synth
    c = synth.registration_pair_c4(20000, seed=3)
    fs, fd = np.ascontiguousarray(c["feat_src"]), np.ascontiguousarray(c["feat_dst"])
    a = m3d.common.KNearestSearch(fd.T).search_knn_batch(fs, 1)[0][:, 0]     # src -> nearest dst
    b = m3d.common.KNearestSearch(fs.T).search_knn_batch(fd, 1)[0][:, 0]     # dst -> nearest src
    src = np.nonzero(b[a] == np.arange(len(fs)))[0]
    s0, s1 = dev.match_mutual_nn(fs, fd)
    order = np.argsort(s0, kind="stable")
    assert np.array_equal(src, s0[order].astype(np.int64)) and np.array_equal(a[src], s1[order].astype(np.int64))


def test_size_full_index(dev, ref):
    from misc3d_amd import synth
    c = synth.registration_pair_c4(200_000, seed=5)
    fs, fd = np.ascontiguousarray(c["feat_src"]), np.ascontiguousarray(c["feat_dst"])
    _same(dev, ref, fd, fs[:500], 10)


CPP = r"""
#include <misc3d/common/knn.h>
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <vector>
int main(int argc, char** argv) {
    std::ifstream f(argv[1], std::ios::binary);
    uint64_t n, dim;
    f.read((char*)&n, 8);
    f.read((char*)&dim, 8);
    std::vector<double> data(n * dim), q(dim);
    f.read((char*)data.data(), 8 * data.size());
    f.read((char*)q.data(), 8 * q.size());
    misc3d::common::KNearestSearch s(data.data(), dim, n, 10);
    std::vector<size_t> idx;
    std::vector<double> dist;
    int k = s.Search(q, misc3d::features::KDTreeSearchParamKNN(7), idx, dist);
    std::printf("%d", k);
    for (size_t i = 0; i < idx.size(); ++i) std::printf(" %zu %a", idx[i], dist[i]);
    std::printf("\n");
    k = s.SearchHybrid(q, 0.8, 20, idx, dist);
    std::printf("%d", k);
    for (size_t i = 0; i < idx.size(); ++i) std::printf(" %zu %a", idx[i], dist[i]);
    std::printf("\n");
    std::vector<double> far(q);
    for (double& v : far) v += 100.0;
    try {
        s.SearchHybrid(far, 0.8, 20, idx, dist);
        std::printf("no throw\n");
    } catch (const std::length_error&) {
        std::printf("length_error\n");
    }
    std::printf("%d %d\n", s.SearchKNN(std::vector<double>(dim + 1), 3, idx, dist),
                s.Search(q, misc3d::features::KDTreeSearchParamRadius(0.5), idx, dist));
    std::vector<size_t> bi;
    std::vector<double> bd;
    std::vector<int64_t> bc;
    s.SearchKNNBatch(q.data(), 1, 7, bi, bd, bc);
    std::printf("%zu %lld\n", bi[0], (long long)bc[0]);
    return 0;
}
"""


def test_cpp_mirror(dev, ref, tmp_path):
    src = tmp_path / "knn_mirror.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "knn_mirror")
    lib = os.path.join(ROOT, "misc3d_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", lib,
                    "-lmisc3d_amd", "-lpthread", "-Wl,-rpath," + lib], check=True)
    rng = np.random.default_rng(11)
    n, dim = 3000, 5
    data = rng.random((n, dim))
    q = rng.random(dim)
    blob = tmp_path / "knn.bin"
    blob.write_bytes(np.array([n, dim], np.uint64).tobytes() + data.tobytes() + q.tobytes())
    r = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")

    def parse(line):
        v = line.split()
        return int(v[0]), [int(x) for x in v[1::2]], [float.fromhex(x) for x in v[2::2]]

    k, i, d = parse(lines[0])
    ri, rd, _, _ = ref.search(data, q, 7)
    nearest = ri[0, 0]
    assert k == 7 and i == ri[0].tolist() and np.array_equal(bits(np.array(d)), bits(rd[0]))
    k, i, d = parse(lines[1])
    ri, rd, _, rc = ref.search(data, q, 20, 2, 0.8)
    assert k == rc[0] and i == ri[0, :k].tolist() and np.array_equal(bits(np.array(d)), bits(rd[0, :k]))
    assert lines[2] == "length_error"
    assert lines[3] == "-1 -1"
    assert lines[4] == f"{nearest} 7"
