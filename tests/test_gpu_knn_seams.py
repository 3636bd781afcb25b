"""KNearestSearch at the seams of its kernels and host loops, on the MI355X: every case equals the plain-C restatement of the
contract (tests/cpp/knn_ref.c) bit for bit -- indices, d2 bits with the canonical NaN, distance bits, hybrid counts.

The hook cases (tests/knn_seam_cases.py) drive launch_knn_tile + launch_knn_merge with a pinned geometry through
m3d_bench_knn_tile_merge: the merge's four lists per lane (S around 64, 128, 192, 256, ragged and empty splits, equal keys in
lists s and s + 64), the 64-query and 4-query workgroups, the list capacities 16 / 32 / 64 / 128, the 32 x 16 LDS tile, the
floor between pages inside a run of equal keys, and lists longer than the data.  The product cases run m3d_knn_search where its
own host loops change: split counts above 64, query chunks of the tile and grid paths, pages x chunks, the chunk halving under
the scratch cap, degenerate density grids, and the first use of every grid class from threads that start together.
tests/test_knn.py shows on a numpy model that these cases notice the faults they are there for."""
import threading
import time

import numpy as np
import pytest

import knn_seam_cases as sc
from knn_ref_util import bits, build_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("knn_ref"))


@pytest.fixture(scope="module")
def dev(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device")
    yield capi
    capi.knn_force_path(0)


def _same(dev, ref, data, queries, knn, search=0, radius=0.0, path=0, index=None, rows=None):
    """C ABI (forced path) == restatement on every query (or on the queries `rows`); returns the stats dict"""
    dev.knn_force_path(path)
    try:
        ix = index or dev.KnnIndex(data)
        i, d, d2, c, st = ix.search(queries, knn, search, radius, stats=True)
    finally:
        dev.knn_force_path(0)
    if rows is not None:
        i, d, d2, c, queries = i[rows], d[rows], d2[rows], c[rows], queries[rows]
    ri, rd, rd2, rc = ref.search(data, queries, knn, search, radius)
    assert np.array_equal(c, rc), (c, rc)
    assert np.array_equal(i, ri), (path, knn, np.argwhere(i != ri)[:5])
    assert np.array_equal(bits(d2), bits(rd2))
    assert np.array_equal(bits(d), bits(rd))
    return st


# ---- through the hook ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", sorted({c.group for c in sc.HOOK_CASES}))
def test_hook_cases(dev, ref, group):
    for c in (c for c in sc.HOOK_CASES if c.group == group):
        data, q = sc.hook_input(c)
        want_i, want_k = sc.hook_expected(ref, c, data, q)
        if sc.expects_lane_lists(c):
            assert sc.reaches_lane_lists(c, want_i, want_k), sc.case_id(c)
        if c.group == "pages":
            assert sc.page_boundary_inside_a_tie(c, want_k), sc.case_id(c)
        got_i, got_k = dev.knn_tile_merge(data, q, c.kk, c.pages, c.S, c.r)
        assert np.array_equal(got_i, want_i), (sc.case_id(c), np.argwhere(got_i != want_i)[:5])
        assert np.array_equal(got_k, want_k), (sc.case_id(c), np.argwhere(got_k != want_k)[:5])
        if c.group == "short":
            real = min(c.n, c.pages * c.kk)          # (n = 40 with 16 pairs is the one list of the family that is full)
            assert np.all(got_i[:, real:] == sc.SENT_IDX) and np.all(got_k[:, real:] == sc.SENT_KEY)
            for row in got_i[:, :real]:
                assert len(np.unique(row)) == real and row.max() < c.n          # no row twice


def test_hook_refuses_bad_geometry(dev):
    data, q = np.zeros((10, 2)), np.zeros((3, 2))
    for kk, pages, S, r in ((0, 1, 1, 10), (129, 1, 1, 10), (1, 0, 1, 10), (1, 1, 0, 10), (1, 1, 257, 10), (1, 1, 1, 0),
                            (1, 1, 3, 3)):
        with pytest.raises(dev.M3DError) as e:
            dev.knn_tile_merge(data, q, kk, pages, S, r)
        assert e.value.code == dev.ERR_INVALID_ARG, (kk, pages, S, r)


# ---- through m3d_knn_search ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (2, 3))
def test_product_split_counts_above_64(dev, ref, dim):
    for n in sc.SPLIT_N:
        data, q = sc.split_input(n, dim)
        ix = dev.KnnIndex(data)
        for k in sc.SPLIT_K:
            st = _same(dev, ref, data, q, k, path=dev.KNN_PATH_TILE if dim == 3 else 0, index=ix)
            assert st["path"] == dev.KNN_PATH_TILE
            assert st["launches"] == 2 and st["pair_dims"] == sc.SPLIT_M * n * dim, (n, k, st)
        ix.close()
    assert [sc.product_geometry(n, sc.SPLIT_M)[0] for n in sc.SPLIT_N] == [64, 65, 129, 193, 256, 256]


@pytest.mark.parametrize("k,launches", ((3, 4), (130, 8)))
def test_tile_chunks_and_pages(dev, ref, k, launches):
    data, q = sc.chunk_input(sc.TILE_CHUNKS, 21)
    assert sc.product_tile_launches(len(data), data.shape[1], len(q), k) == launches
    st = _same(dev, ref, data, q, k)
    assert st["path"] == (dev.KNN_PATH_TILE if k <= 128 else dev.KNN_PATH_SELECT)
    assert st["launches"] == launches, st


def test_chunk_halving_under_the_scratch_cap(dev, ref):
    """16 408 bytes of scratch per query at S = 8 against 16 384 allowed at 16 384 queries: chunks of 8 192, 8 192 and 1."""
    s = sc.HALVING
    assert sc.product_chunk(s["n"], s["dim"], s["m"], s["k"]) == 8192
    data, q = sc.chunk_input(s, 22)
    rows = np.unique(np.concatenate([[0, 8191, 8192, 16383, 16384], np.random.default_rng(23).integers(0, s["m"], 200)]))
    t0 = time.perf_counter()
    st = _same(dev, ref, data, q, s["k"], rows=rows)
    print("halving case: %.2f s with the reference on %d rows, device %.1f ms" % (time.perf_counter() - t0, len(rows), st["ms_device"]))
    assert st["path"] == dev.KNN_PATH_TILE and st["launches"] == 6, st
    assert st["pair_dims"] == s["m"] * s["n"] * s["dim"]


@pytest.mark.parametrize("k", (1, 17))
def test_grid_chunks(dev, ref, k):
    s = sc.GRID_CHUNKS
    data, q = sc.chunk_input(s, 24)
    for row, v in sc.GRID_CHUNK_NONFINITE:
        q[row, row % 3] = v
    ix = dev.KnnIndex(data)
    st = _same(dev, ref, data, q, k, index=ix)
    assert st["path"] == dev.KNN_PATH_GRID and st["tile_queries"] == 3 and st["launches"] == 2 + 2, st
    # HYBRID: the radius is the median distance of the middle neighbour, so about half of the lists are cut
    _, rd, _, _ = ref.search(data, q[:2000], k)
    radius = float(np.nanmedian(rd[:, k // 2]))
    st = _same(dev, ref, data, q, k, search=dev.KNN_SEARCH_HYBRID, radius=radius, index=ix)
    assert st["tile_queries"] == 3 and st["launches"] == 4, st
    ix.close()


@pytest.mark.parametrize("name", sc.DEGENERATE)
def test_degenerate_grids(dev, ref, name):
    rows = sc.degenerate_rows(name)
    ix = dev.KnnIndex(rows)
    for t, k in enumerate(sc.DEGENERATE_K):
        q = sc.degenerate_queries(rows, (63, 64, 65)[t % 3])
        for path in (0, dev.KNN_PATH_TILE):
            st = _same(dev, ref, rows, q, k, path=path, index=ix)
            assert st["path"] == (path or dev.KNN_PATH_GRID), (name, k, st)
    ix.close()


def test_fewer_finite_rows_than_the_list(dev, ref):
    rows = sc.degenerate_rows("nonfinite")
    assert len(rows) == 40 and np.isfinite(rows).all(axis=1).sum() == 30
    ix = dev.KnnIndex(rows)
    for count in (63, 64, 65):
        q = sc.degenerate_queries(rows, count)
        for path in (0, dev.KNN_PATH_TILE):
            st = _same(dev, ref, rows, q, 40, path=path, index=ix)
            assert st["path"] == (path or dev.KNN_PATH_GRID)
            i, _, d2, _ = ix.search(q, 40)
            for qi in np.nonzero(np.isfinite(q).all(axis=1))[0]:
                fin, inf, nan = np.isfinite(d2[qi]), np.isposinf(d2[qi]), np.isnan(d2[qi])
                assert fin[:30].all() and inf[30:35].all() and nan[35:].all()          # +inf before NaN ...
                assert np.all(np.diff(i[qi, 30:35]) > 0) and np.all(np.diff(i[qi, 35:]) > 0)   # ... each in index order
    ix.close()


def test_first_use_of_every_grid_class_from_threads(dev, ref):
    rng = np.random.default_rng(25)
    data = rng.standard_normal((5000, 3))
    ks = (5, 5, 20, 20, 50, 50, 100, 100)
    qs = [rng.standard_normal((40, 3)) for _ in ks]
    ix = dev.KnnIndex(data)
    out, err = [None] * len(ks), []
    gate = threading.Barrier(len(ks))

    def run(j):
        try:
            gate.wait(timeout=30)
            out[j] = ix.search(qs[j], ks[j], stats=True)
        except Exception as e:          # noqa: BLE001 -- reported below, in the main thread
            err.append((j, repr(e)))

    th = [threading.Thread(target=run, args=(j,)) for j in range(len(ks))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for j, k in enumerate(ks):
        i, d, d2, c, st = out[j]
        ri, rd, rd2, rc = ref.search(data, qs[j], k)
        assert st["path"] == dev.KNN_PATH_GRID
        assert np.array_equal(i, ri) and np.array_equal(c, rc), (j, k)
        assert np.array_equal(bits(d2), bits(rd2)) and np.array_equal(bits(d), bits(rd))
    ix.close()
