"""KNearestSearch without a device: the plain-C restatement of the contract (tests/cpp/knn_ref.c) against numpy brute force
and scipy, its hybrid quirks, the exported C ABI and its argument checks, and the python class's device-free paths."""
import ctypes as C
import inspect

import numpy as np
import pytest

from knn_ref_util import bits, build_ref, numpy_brute


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("knn_ref"))


def test_restatement_equals_numpy(ref):
    rng = np.random.default_rng(0)
    for dim, n, knn in ((1, 300, 7), (3, 2000, 30), (33, 1500, 10), (5, 200, 250), (3, 50, 60)):
        data = rng.standard_normal((n, dim))
        data[:20] = data[20:40]                              # duplicates
        data[3, 0], data[4, dim - 1], data[5] = np.nan, np.inf, 1e200
        q = rng.standard_normal((12, dim))
        q[0, 0] = np.nan
        q[1] = data[25]
        i, _, d2, c = ref.search(data, q, knn)
        with np.errstate(over="ignore", invalid="ignore"):
            ni, nd2 = numpy_brute(data, q, knn)
        assert np.array_equal(i, ni)
        assert np.array_equal(bits(d2), bits(nd2))
        assert (c == min(knn, n)).all()


def test_restatement_equals_scipy(ref):
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(1)
    for dim in (3, 8):
        data = rng.random((5000, dim))
        q = rng.random((200, dim))
        i, d, _, _ = ref.search(data, q, 9)
        sd, si = cKDTree(data).query(q, 9)
        assert np.array_equal(i, si)
        assert np.allclose(d, sd, rtol=1e-14, atol=0)


def test_restatement_hybrid_quirks(ref):
    data = np.array([[0.0], [1.0], [2.0], [3.0], [10.0]])
    q = np.array([[0.0]])

    def hyb(knn, r):
        i, d, _, c = ref.search(data, q, knn, 2, r)
        return int(c[0]), i[0, :max(int(c[0]), 0)].tolist()

    assert hyb(5, 2.5) == (2, [0, 1])         # 3 inside, the last in-radius one dropped
    assert hyb(5, 100.0) == (4, [0, 1, 2, 3])  # none beyond: i = kout, still one dropped
    assert hyb(5, 0.5) == (0, [])              # one inside -> num 0 -> nothing
    assert hyb(5, -1.0) == (-1, [])            # nearest beyond the radius: the size_t wrap
    assert hyb(0, 1.0) == (-1, [])             # knn == 0: i == 0 as well
    assert hyb(5, float("nan")) == (4, [0, 1, 2, 3])   # NaN radius: nothing compares greater
    d = data.copy()
    d[1, 0] = np.nan                                   # a NaN distance counts as inside
    i, _, _, c = ref.search(d, q, 5, 2, 100.0)           # NaN ranks last and is not "beyond": i = kout
    assert int(c[0]) == 4 and i[0, :4].tolist() == [0, 2, 3, 4]


NAMES = ("m3d_knn_create", "m3d_knn_destroy", "m3d_knn_size", "m3d_knn_dim", "m3d_knn_search", "m3d_bench_knn_force_path")


def test_exports_and_header(capi):
    L = capi.lib()
    for name in NAMES:
        assert hasattr(L, name), name
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "misc3d_amd.h")).read() + open(os.path.join(root, "include",
                                                                                        "misc3d_amd_bench.h")).read()
    for name in NAMES:
        assert name + "(" in hdr, name


def test_create_argument_errors(capi):
    tiny = np.zeros(4)
    p = tiny.ctypes.data_as(C.c_void_p)
    assert capi.knn_create_status(p, 1, 0)[0] == -5
    assert capi.knn_create_status(p, 1, 1025)[0] == -5
    assert capi.knn_create_status(p, 2**31, 1)[0] == -5
    assert capi.knn_create_status(p, 0, 3)[0] == -5
    assert capi.knn_create_status(None, 10, 3)[0] == -5
    assert capi.lib().m3d_knn_search(None, None, 0, 0, 1, 0.0, 0, None, None, None, None, None) == -5
    assert capi.lib().m3d_knn_size(None) == 0 and capi.lib().m3d_knn_dim(None) == 0
    assert capi.lib().m3d_bench_knn_force_path(7) == -5


def test_python_class_without_device():
    import misc3d_amd as m3d
    K = m3d.common.KNearestSearch
    s = K()
    q = np.zeros(3)
    assert s.search_knn(q, 5) == ([], [])
    assert s.search_hybrid(q, 1.0, 5) == ([], [])
    assert s.search(q, ("knn", 3)) == ([], []) and s.search(q, ("hybrid", 1.0, 3)) == ([], [])
    assert s.search(q, ("radius", 1.0)) == ([], [])
    assert s.set_mat_data(np.zeros((0, 4))) is False and s.set_mat_data(np.zeros((3, 0))) is False
    assert s.set_geometry(object()) is False
    assert K(7).search_knn(q, 1) == ([], [])
    for f in (s.search_knn_batch,):
        with pytest.raises(ValueError):
            f(np.zeros((2, 3)), 3)
    with pytest.raises(ValueError):
        s.search_hybrid_batch(np.zeros((2, 3)), 1.0, 3)


def test_python_signatures():
    import misc3d_amd as m3d
    K = m3d.common.KNearestSearch
    doc = K.__init__.__doc__
    assert "__init__(self: misc3d_amd._py_misc3d.common.KNearestSearch, *, device" in doc
    assert "n_trees: typing.SupportsInt" in doc or "n_trees: int" in doc
    assert "data: numpy.ndarray, n_trees: " in doc and "= 10, *, device" in doc
    assert "geometry: object, n_trees: " in doc and "= 4, *, device" in doc
    for name, args in (("set_mat_data", ["data"]), ("set_geometry", ["geometry"]), ("set_feature", ["feature"]),
                       ("search", ["query", "param"]), ("search_knn", ["query", "knn"]),
                       ("search_hybrid", ["query", "radius", "knn"]), ("search_knn_batch", ["queries", "knn"]),
                       ("search_hybrid_batch", ["queries", "radius", "knn"])):
        d = getattr(K, name).__doc__
        assert d.startswith(name + "(self: misc3d_amd._py_misc3d.common.KNearestSearch, " + args[0]), d
        for a in args:
            assert a + ":" in d.split("->")[0], (name, a)
