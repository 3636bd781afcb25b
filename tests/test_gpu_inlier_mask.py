"""RefineModel's inlier list shipped as a bit mask and expanded on the host (m3d_config.list_mask, default 1) against the
device writing the list itself (list_mask 0): the same return code, bit-identical parameters, the same statistics and the
same list, element for element -- at the C2 size, on edge clouds, for spheres and with several threads on several lanes."""
import threading

import numpy as np
import pytest

from misc3d_amd import synth

pytestmark = pytest.mark.gpu

STATS = ("count", "iterations", "best_index", "general_fit_ok", "n_inliers", "fitness", "inlier_rmse")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _fit(capi, pts, kind, thr, H, seed, list_mask, copy=True):
    old = capi.set_config(list_mask=list_mask)
    try:
        with capi.Cloud(pts) as c:
            g = c.fit(kind, thr, H, 1.0, seed=seed, copy=copy)
            return g.ret, np.array(g.params, copy=True), np.array(g.inliers, copy=True), {k: g.stats.get(k) for k in STATS}
    finally:
        capi.restore_config(old)


def _fit_or_error(capi, *args):
    try:
        return _fit(capi, *args)
    except capi.M3DError as e:
        return ("error", str(e))


def _same(a, b):
    if a[0] == "error" or b[0] == "error":
        assert a == b
        return
    assert a[0] == b[0]
    assert np.array_equal(_bits(a[1]), _bits(b[1]))
    assert a[2].dtype == b[2].dtype and np.array_equal(a[2], b[2])
    for k in STATS:
        va, vb = a[3][k], b[3][k]
        assert (va == vb) or (isinstance(va, float) and np.isnan(va) and np.isnan(vb)), (k, va, vb)


@pytest.mark.parametrize("copy", [False, True])
def test_c2_full_size_mask_equals_device_list(capi, copy):
    pts = synth.plane_cloud_c2(1_000_000, seed=2)
    new = _fit(capi, pts, 0, 0.01, 10_000, 11, 1, copy)
    old = _fit(capi, pts, 0, 0.01, 10_000, 11, 0, copy)
    _same(new, old)
    assert 0.45 * len(pts) < len(new[2]) < 0.56 * len(pts)
    assert np.all(np.diff(new[2].astype(np.int64)) > 0)


@pytest.mark.parametrize("n", [2048 - 1, 2048 + 1, 5 * 2048 - 1, 5 * 2048, 5 * 2048 + 1, 40_000 + 3])
def test_tile_edges(capi, n):
    pts = synth.plane_cloud_c1(n, 3)
    _same(_fit(capi, pts, 0, 0.01, 300, 5, 1), _fit(capi, pts, 0, 0.01, 300, 5, 0))


@pytest.mark.parametrize("thr", [1e-300, 1e6])
def test_no_inlier_and_every_point(capi, thr):
    pts = synth.plane_cloud_c1(20_000 + 17, 4)
    a, b = _fit(capi, pts, 0, thr, 200, 9, 1), _fit(capi, pts, 0, thr, 200, 9, 0)
    _same(a, b)
    if thr > 1:
        assert len(a[2]) == len(pts)


@pytest.mark.parametrize("n", [3, 4, 5])
def test_tiny_clouds(capi, n):
    rng = np.random.default_rng(n)
    pts = rng.random((n, 3))
    pts[:, 2] = 0.25
    _same(_fit_or_error(capi, pts, 0, 0.01, 50, 1, 1), _fit_or_error(capi, pts, 0, 0.01, 50, 1, 0))


def test_only_the_first_or_the_last_point_off_the_plane(capi):
    n = 3 * 2048 + 5
    for off in (0, n - 1):
        rng = np.random.default_rng(off)
        pts = rng.random((n, 3))
        pts[:, 2] = 0.0
        pts[off, 2] = 5.0
        a, b = _fit(capi, pts, 0, 0.01, 100, 2, 1), _fit(capi, pts, 0, 0.01, 100, 2, 0)
        _same(a, b)
        assert off not in set(a[2].tolist()) and len(a[2]) == n - 1


def test_sphere(capi):
    pts = synth.sphere_cloud_c3(200_000, 4)
    _same(_fit(capi, pts, 1, 0.01, 2000, 7, 1), _fit(capi, pts, 1, 0.01, 2000, 7, 0))


def test_threads_on_lanes(capi):
    clouds = [synth.plane_cloud_c2(300_000 + 1000 * i, seed=3 + i) for i in range(6)]
    serial = [_fit(capi, p, 0, 0.01, 3000, 21 + i, 1) for i, p in enumerate(clouds)]
    out = [None] * len(clouds)
    errs = []

    def run(i):
        try:
            with capi.Cloud(clouds[i]) as c:
                for _ in range(3):
                    g = c.fit(0, 0.01, 3000, 1.0, seed=21 + i)
                    r = (g.ret, np.array(g.params, copy=True), np.array(g.inliers, copy=True), {k: g.stats.get(k) for k in STATS})
                    if out[i] is None:
                        out[i] = r
                    _same(r, out[i])
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=run, args=(i,)) for i in range(len(clouds))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for a, b in zip(out, serial):
        _same(a, b)
