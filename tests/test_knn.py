"""KNearestSearch without a device: the plain-C restatement of the contract (tests/cpp/knn_ref.c) against numpy brute force
and scipy, its hybrid quirks, the exported C ABI and its argument checks, and the python class's device-free paths; and a
numpy model of the tile path (split lists, floor, a merge with four lists per lane, query chunks) that equals the restatement on
the cases of tests/test_gpu_knn_seams.py and, with one fault planted at a time, differs on the cases named for that fault."""
import ctypes as C
import inspect

import numpy as np
import pytest

import knn_seam_cases as sc
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


# ---- the seam cases of tests/test_gpu_knn_seams.py notice the faults they are there for ------------------------------------
# A numpy model of the tile path as m3d_knn.hip / m3d_knn.cpp lay it out: per split a sorted list of kk pairs above the floor,
# a merge in which lane l owns the lists l, l + 64, l + 128, l + 192 and the wavefront takes the smallest head kk times, the
# last pair of a page as the next page's floor, and chunks of queries, each laid out as qT with the chunk's own stride.
FAULTS = ("drop_last_row",        # the last row of a split is never offered
          "ignore_lists_64_up",   # the merge reads a lane's first list only
          "tie_larger_index",     # equal keys: the larger index first
          "floor_key_only",       # a page keeps key > floor key, not (key, index) > floor
          "chunk_stride")         # a later chunk's qT is read with the first chunk's stride
_ONES = np.uint64(sc.SENT_KEY)


def _model_keys(data, q):
    acc = np.zeros((len(q), len(data)))
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(data.shape[1]):
            d = q[:, k, None] - data[None, :, k]
            acc = acc + d * d
    return bits(acc)


def _model_sorted(key, idx, kk, fault):
    """the kk smallest (key, index) of each row of key / idx (sentinels last), padded with sentinels"""
    m = len(key)
    tie = -idx if fault == "tie_larger_index" else idx
    order = np.lexsort((tie, key), axis=1)[:, :kk]
    out_k = np.full((m, kk), _ONES, np.uint64)
    out_i = np.full((m, kk), sc.SENT_IDX, np.int64)
    out_k[:, :order.shape[1]] = np.take_along_axis(key, order, 1)
    out_i[:, :order.shape[1]] = np.take_along_axis(idx, order, 1)
    return out_k, out_i


def _model_split_lists(keys, kk, S, r, floor, fault):
    m, n = keys.shape
    part_k = np.full((m, S, kk), _ONES, np.uint64)
    part_i = np.full((m, S, kk), sc.SENT_IDX, np.int64)
    for s in range(S):
        r0, r1 = min(s * r, n), min(s * r + r, n)
        if fault == "drop_last_row" and r1 > r0:
            r1 -= 1
        key = keys[:, r0:r1].copy()
        idx = np.broadcast_to(np.arange(r0, r1, dtype=np.int64), key.shape).copy()
        if floor is not None:
            fk, fi = floor[0][:, None], floor[1][:, None]
            above = key > fk
            if fault != "floor_key_only":
                above |= (key == fk) & (idx > fi)
            key[~above] = _ONES
            idx[~above] = sc.SENT_IDX
        part_k[:, s], part_i[:, s] = _model_sorted(key, idx, kk, fault)
    return part_k, part_i


def _model_merge(part_k, part_i, fault):
    m, S, kk = part_k.shape
    lists = 64 if fault == "ignore_lists_64_up" else 256
    hk = np.full((m, 256, kk + 1), _ONES, np.uint64)          # (column kk: a list that is used up)
    hi = np.full((m, 256, kk + 1), sc.SENT_IDX, np.int64)
    hk[:, :min(S, lists), :kk] = part_k[:, :lists]
    hi[:, :min(S, lists), :kk] = part_i[:, :lists]
    pos = np.zeros((m, 256), np.int64)
    out_k = np.zeros((m, kk), np.uint64)
    out_i = np.zeros((m, kk), np.int64)
    larger = fault == "tie_larger_index"

    def smallest(k, i, axis):
        """the smallest (key, index) along an axis and where it is"""
        kmin = k.min(axis=axis, keepdims=True)
        cand = np.where(k == kmin, -i if larger else i, np.iinfo(np.int64).max)
        at = cand.argmin(axis=axis)
        return np.take_along_axis(k, np.expand_dims(at, axis), axis).squeeze(axis), \
            np.take_along_axis(i, np.expand_dims(at, axis), axis).squeeze(axis), at

    for o in range(kk):
        k = np.take_along_axis(hk, pos[:, :, None], 2)[:, :, 0].reshape(m, 4, 64)          # [j][lane]: list lane + 64 j
        i = np.take_along_axis(hi, pos[:, :, None], 2)[:, :, 0].reshape(m, 4, 64)
        bk, bi, bj = smallest(k, i, 1)                  # every lane: the smallest of its four heads
        mk, mi, lane = smallest(bk, bi, 1)              # the wavefront: the smallest of the lanes'
        out_k[:, o], out_i[:, o] = mk, mi
        real = mi != sc.SENT_IDX                        # (a sentinel head has no owner: nothing advances)
        owner = np.take_along_axis(bj, lane[:, None], 1)[:, 0] * 64 + lane
        pos[np.nonzero(real)[0], owner[real]] += 1
    return out_k, out_i


def model_chunk(data, q, kk, pages, S, r, fault=None):
    """what m3d_bench_knn_tile_merge returns -> (indices uint32, key bits uint64), each (m, pages kk)"""
    keys = _model_keys(data, q)
    out_i = np.zeros((len(q), pages * kk), np.uint32)
    out_k = np.zeros((len(q), pages * kk), np.uint64)
    floor = None
    for p in range(pages):
        pk, pi = _model_merge(*_model_split_lists(keys, kk, S, r, floor, fault), fault)
        out_k[:, p * kk:(p + 1) * kk], out_i[:, p * kk:(p + 1) * kk] = pk, pi
        floor = (pk[:, -1], pi[:, -1])
    return out_i, out_k


def model_search(data, queries, k, chunk, fault=None, edge=64):
    """run_tile: chunks of `chunk` queries, each transposed with its own stride, one page; the model evaluates the first and
    last `edge` queries of every chunk (queries are independent) -> (their query numbers, indices, key bits)"""
    m, dim = queries.shape
    rows, out_i, out_k = [], [], []
    stride0 = min(chunk, m)
    for c0 in range(0, m, chunk):
        mc = min(chunk, m - c0)
        qT = np.ascontiguousarray(queries[c0:c0 + mc].T).ravel()          # [k mc + q]
        stride = stride0 if fault == "chunk_stride" else mc
        lanes = np.unique(np.concatenate([np.arange(min(edge, mc)), np.arange(max(mc - edge, 0), mc)]))
        at = (np.arange(dim)[None, :] * stride + lanes[:, None]) % qT.size   # (the model wraps; a kernel would not)
        S, r = sc.product_geometry(len(data), mc)
        i, key = model_chunk(data, qT[at], k, 1, S, r, fault)
        rows.append(c0 + lanes)
        out_i.append(i)
        out_k.append(key)
    return np.concatenate(rows), np.concatenate(out_i), np.concatenate(out_k)


def _hook_differs(ref, c, fault=None):
    data, q = sc.hook_input(c)
    want = sc.hook_expected(ref, c, data, q)
    got = model_chunk(data, q, c.kk, c.pages, c.S, c.r, fault)
    return not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))


@pytest.mark.parametrize("group", sorted({c.group for c in sc.HOOK_CASES}))
def test_model_equals_restatement_on_the_hook_cases(ref, group):
    for c in (c for c in sc.HOOK_CASES if c.group == group):
        data, q = sc.hook_input(c)
        want_i, want_k = sc.hook_expected(ref, c, data, q)
        if sc.expects_lane_lists(c):
            assert sc.reaches_lane_lists(c, want_i, want_k), sc.case_id(c)
        if c.group == "pages":
            assert sc.page_boundary_inside_a_tie(c, want_k), sc.case_id(c)
        assert not _hook_differs(ref, c), sc.case_id(c)


def test_hook_cases_cover_what_the_issue_names():
    cases = [c for c in sc.HOOK_CASES if c.group == "merge"]
    for S in sc.MERGE_S:
        mine = [c for c in cases if c.S == S]
        assert {c.r for c in mine} == set(sc.MERGE_R) and {c.kk for c in mine} == set(sc.MERGE_KK)
        assert {c.family for c in mine} == {"random", "ties"}
        if S > 2:          # a full, a ragged and a two-empty-splits n (at r = 1 the ragged n is the full one)
            assert any(c.n == S * c.r for c in mine) and any(c.n == (S - 2) * c.r for c in mine)
            assert any(c.n == S * c.r - (c.r - 1) for c in mine)
    assert sum(sc.expects_lane_lists(c) for c in cases) >= 8
    assert {c.m for c in sc.HOOK_CASES if c.group == "qblock"} == {1, 3, 4, 5, 63, 64, 65, 129}
    assert {c.kk for c in sc.HOOK_CASES if c.group == "kcap"} == {15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128}
    assert {c.dim for c in sc.HOOK_CASES if c.group == "tile_dim"} == {1, 15, 16, 17, 31, 32, 33, 48, 49}
    assert {c.n for c in sc.HOOK_CASES if c.group == "tile_rows" and c.S == 1} == {31, 32, 33, 63, 64, 65}
    assert any(c.r % sc.TILE_ROWS and c.S == 4 for c in sc.HOOK_CASES if c.group == "tile_rows")
    assert {(c.pages, c.kk) for c in sc.HOOK_CASES if c.group == "pages"} == {(p, k) for p in (2, 3) for k in (1, 16, 17)}
    short = [c for c in sc.HOOK_CASES if c.group == "short"]
    assert {(c.n, c.pages * c.kk) for c in short} == {(n, w) for n in (1, 5, 40) for w in (16, 48, 128)}
    assert all(c.pages * c.kk > c.n for c in short if (c.n, c.pages * c.kk) != (40, 16))   # (the one list that is full)
    for c in sc.HOOK_CASES:
        assert c.S * c.r >= c.n and 1 <= c.S <= sc.MAX_SPLITS and 1 <= c.kk <= sc.PAGE_MAX


# the named cases every fault must fail (the cheap ones first); test_every_fault_is_noticed also counts all the hook cases
_NAMED = {
    "drop_last_row": [c for c in sc.HOOK_CASES if c.group == "tile_rows"],
    "ignore_lists_64_up": [c for c in sc.HOOK_CASES if c.group == "merge" and c.S in (65, 129, 193, 256)],
    "tie_larger_index": [c for c in sc.HOOK_CASES if c.family == "ties"],
    "floor_key_only": [c for c in sc.HOOK_CASES if c.group == "pages"],
}


@pytest.mark.parametrize("fault", [f for f in FAULTS if f != "chunk_stride"])
def test_every_fault_is_noticed_by_its_hook_cases(ref, fault):
    hit = [sc.case_id(c) for c in _NAMED[fault] if _hook_differs(ref, c, fault)]
    print(fault, "->", len(hit), "of", len(_NAMED[fault]), "named cases")
    assert hit, fault
    if fault == "ignore_lists_64_up":      # every case that claims to reach a lane's second list notices the lists' loss
        for c in (c for c in sc.HOOK_CASES if sc.expects_lane_lists(c)):
            assert _hook_differs(ref, c, fault), sc.case_id(c)
        assert not any(_hook_differs(ref, c, fault) for c in sc.HOOK_CASES if c.S <= 64)
    if fault == "floor_key_only":          # every page case: its boundary lies inside a run of equal keys
        assert len(hit) == len(_NAMED[fault])


def test_a_stale_chunk_stride_is_noticed_by_the_tile_chunk_case(ref):
    """the product case of test_tile_chunks_and_pages (two chunks, 16 384 + 1 queries): the model with the real chunk size
    equals the restatement, and with the first chunk's stride in the second chunk it does not -- in the last query alone"""
    data, q = sc.chunk_input(sc.TILE_CHUNKS, 21)
    k = 3
    rows, gi, gk = model_search(data, q, k, sc.TILE_CHUNK)
    assert rows.tolist() == list(range(64)) + list(range(sc.TILE_CHUNK - 64, sc.TILE_CHUNK + 1))
    ri, _, rd2, _ = ref.search(data, q[rows], k)
    assert np.array_equal(gi, ri) and np.array_equal(gk, bits(rd2))
    _, fi, fk = model_search(data, q, k, sc.TILE_CHUNK, "chunk_stride")
    assert np.array_equal(fi[:-1], ri[:-1]) and np.array_equal(fk[:-1], bits(rd2)[:-1])
    assert not np.array_equal(fk[-1], bits(rd2)[-1])


def test_product_shapes_reach_what_they_name():
    """the shapes of the product cases follow from run_tile's two lambdas as knn_seam_cases restates them"""
    assert [sc.product_geometry(n, sc.SPLIT_M)[0] for n in sc.SPLIT_N] == [64, 65, 129, 193, 256, 256]
    t = sc.TILE_CHUNKS
    assert sc.product_chunk(t["n"], t["dim"], t["m"], 3) == sc.TILE_CHUNK
    assert sc.product_tile_launches(t["n"], t["dim"], t["m"], 3) == 4
    assert sc.product_tile_launches(t["n"], t["dim"], t["m"], 130) == 8
    h = sc.HALVING
    assert sc.product_geometry(h["n"], sc.TILE_CHUNK) == (8, 449)
    per_query = h["dim"] * 8 + 8 * h["k"] * 12 + h["k"] * 12 + 16
    assert per_query == 16408 and per_query * sc.TILE_CHUNK > sc.SCRATCH_CAP >= per_query * 8192
    assert sc.product_chunk(h["n"], h["dim"], h["m"], h["k"]) == 8192
    assert sc.product_tile_launches(h["n"], h["dim"], h["m"], h["k"]) == 6


def test_tile_merge_hook_checks_its_arguments(capi):
    data, q = np.zeros((10, 2)), np.zeros((3, 2))
    for kk, pages, S, r in ((0, 1, 1, 10), (129, 1, 1, 10), (1, 0, 1, 10), (1, 1, 0, 10), (1, 1, 257, 10), (1, 1, 1, 0),
                            (1, 1, 3, 3), (1, 1, 9, 1)):
        with pytest.raises(capi.M3DError) as e:
            capi.knn_tile_merge(data, q, kk, pages, S, r)
        assert e.value.code == capi.ERR_INVALID_ARG, (kk, pages, S, r)
    L = capi.lib()
    p = data.ctypes.data_as(C.c_void_p)
    assert L.m3d_bench_knn_tile_merge(p, 10, 0, p, 3, 1, 1, 1, 10, 0, p, p) == capi.ERR_INVALID_ARG
    assert L.m3d_bench_knn_tile_merge(p, 10, 1025, p, 3, 1, 1, 1, 10, 0, p, p) == capi.ERR_INVALID_ARG
    assert L.m3d_bench_knn_tile_merge(p, 0, 2, p, 3, 1, 1, 1, 10, 0, p, p) == capi.ERR_INVALID_ARG
    assert L.m3d_bench_knn_tile_merge(p, 10, 2, p, 0, 1, 1, 1, 10, 0, p, p) == capi.ERR_INVALID_ARG
    assert L.m3d_bench_knn_tile_merge(None, 10, 2, p, 3, 1, 1, 1, 10, 0, p, p) == capi.ERR_INVALID_ARG
    if capi.device_count() == 0:          # a valid call without a device fails, loudly
        with pytest.raises(capi.M3DError) as e:
            capi.knn_tile_merge(data, q, 1, 1, 1, 10)
        assert e.value.code == capi.ERR_DEVICE


NAMES = ("m3d_knn_create", "m3d_knn_destroy", "m3d_knn_size", "m3d_knn_dim", "m3d_knn_search", "m3d_bench_knn_force_path",
         "m3d_bench_knn_tile_merge")


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
