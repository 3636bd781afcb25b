"""The mask form's early expansion (m3d_config.mask_early, default 1): the host writes the inlier list as soon as the mask and
the tile counts are in its memory -- announced by the "mask ready" word, ahead of the moments and the total -- against the
order of mask_early 0 (the completion word first) and against the device writing the list itself (list_mask 0).  Everything is
compared exactly: the return code, the parameter bits, the whole list and the integer statistics."""
import threading

import numpy as np
import pytest

from misc3d_amd import synth

pytestmark = pytest.mark.gpu

STATS = ("count", "iterations", "best_index", "general_fit_ok", "n_inliers", "fitness", "inlier_rmse")
# (list_mask, mask_early): the new order, the order before it, the device's own list
FORMS = ((1, 1), (1, 0), (0, 1))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _result(g):
    inl = None if g.inliers is None else np.array(g.inliers, copy=True)
    return g.ret, np.array(g.params, copy=True), inl, {k: g.stats.get(k) for k in STATS}


def _fit(capi, pts, kind, thr, H, seed, form, copy=True, want_inliers=True):
    old = capi.set_config(list_mask=form[0], mask_early=form[1])
    try:
        with capi.Cloud(pts) as c:
            return _result(c.fit(kind, thr, H, 1.0, seed=seed, copy=copy, want_inliers=want_inliers))
    finally:
        capi.restore_config(old)


def _fit_or_error(capi, *args, **kw):
    try:
        return _fit(capi, *args, **kw)
    except capi.M3DError as e:
        return ("error", str(e))


def _same(a, b):
    if a[0] == "error" or b[0] == "error":
        assert a == b
        return
    assert a[0] == b[0]
    assert np.array_equal(_bits(a[1]), _bits(b[1]))
    if a[2] is None or b[2] is None:
        assert a[2] is None and b[2] is None
    else:
        assert a[2].dtype == b[2].dtype and np.array_equal(a[2], b[2])
    for k in STATS:
        va, vb = a[3][k], b[3][k]
        assert (va == vb) or (isinstance(va, float) and np.isnan(va) and np.isnan(vb)), (k, va, vb)


def _all_forms_agree(capi, *args, **kw):
    out = [_fit_or_error(capi, *args, form=f, **kw) for f in FORMS]
    _same(out[0], out[1])
    _same(out[0], out[2])
    return out[0]


def test_switch_defaults_to_on_and_takes_both_values(capi):
    assert capi.get_config().mask_early == 1
    old = capi.set_config(mask_early=0)
    try:
        assert capi.get_config().mask_early == 0
        capi.set_config(mask_early=7)
        assert capi.get_config().mask_early == 1
    finally:
        capi.restore_config(old)
    assert capi.get_config().mask_early == 1


@pytest.mark.parametrize("copy", [False, True])
def test_c2_full_size(capi, copy):
    pts = synth.plane_cloud_c2(1_000_000, seed=2)
    r = _all_forms_agree(capi, pts, 0, 0.01, 10_000, 11, copy=copy)
    assert 0.45 * len(pts) < len(r[2]) < 0.56 * len(pts)
    assert np.all(np.diff(r[2].astype(np.int64)) > 0)


def test_c2_repeated_fits_on_one_cloud(capi):
    """the words of h_sync carry a new sequence value per fit: the second and third fit must not take the first one's"""
    pts = synth.plane_cloud_c2(1_000_000, seed=5)
    ref = [_fit(capi, pts, 0, 0.01, 3000, 40 + k, (0, 1)) for k in range(3)]
    with capi.Cloud(pts) as c:
        for rep in range(2):
            for k in range(3):
                _same(_result(c.fit(0, 0.01, 3000, 1.0, seed=40 + k)), ref[k])


@pytest.mark.parametrize("n", [2048 - 1, 2048 + 1, 5 * 2048 - 1, 5 * 2048, 5 * 2048 + 1, 40_000 + 3])
def test_tile_edges(capi, n):
    pts = synth.plane_cloud_c1(n, 3)
    _all_forms_agree(capi, pts, 0, 0.01, 300, 5)


@pytest.mark.parametrize("thr", [1e-300, 1e6])
def test_no_inlier_and_every_point(capi, thr):
    pts = synth.plane_cloud_c1(20_000 + 17, 4)
    r = _all_forms_agree(capi, pts, 0, thr, 200, 9)
    if thr > 1:
        assert len(r[2]) == len(pts)


def test_sphere(capi):
    pts = synth.sphere_cloud_c3(200_000, 4)
    _all_forms_agree(capi, pts, 1, 0.01, 2000, 7)


def test_without_the_list(capi):
    pts = synth.plane_cloud_c2(300_000, seed=6)
    r = _all_forms_agree(capi, pts, 0, 0.01, 3000, 13, want_inliers=False)
    full = _fit(capi, pts, 0, 0.01, 3000, 13, (1, 1))
    assert len(r[2]) == 0 and len(full[2]) == full[3]["n_inliers"] > 0
    _same(r, (full[0], full[1], r[2], full[3]))


def test_early_pick_redone(capi):
    """tests/test_gpu_parity.py's two sheets of equal inlier count: the replay overrules the device's early pick, the mask
    compaction queued on it drains unread and RefineModel is queued again -- with the next sequence value"""
    rng = np.random.default_rng(12)
    n = 4000
    xy = rng.uniform(-1, 1, (n, 2))
    z = np.where(np.arange(n) % 2 == 0, 0.0 + rng.uniform(-4e-3, 4e-3, n), 0.5 + rng.uniform(-1e-3, 1e-3, n))
    pts = np.ascontiguousarray(np.c_[xy, z])
    pts[0], pts[2], pts[4] = (-1, -1, 0.0), (1, -1, 0.0), (0, 1, 0.0)
    pts[1], pts[3], pts[5] = (-1, -1, 0.5), (1, -1, 0.5), (0, 1, 0.5)
    redone = 0
    for seed in range(12):
        out = []
        for form in FORMS:
            old = capi.set_config(list_mask=form[0], mask_early=form[1])
            try:
                with capi.Cloud(pts) as c:
                    g = c.fit(0, 0.01, 1500, 1.0, seed=seed)
                    out.append(_result(g))
                    if form == (1, 1):
                        redone += int(g.stats["early_pick_redone"])
            finally:
                capi.restore_config(old)
        _same(out[0], out[1])
        _same(out[0], out[2])
    assert redone > 0


def test_threads_on_lanes(capi):
    clouds = [synth.plane_cloud_c2(300_000 + 1000 * i, seed=3 + i) for i in range(6)]
    serial = [_fit(capi, p, 0, 0.01, 3000, 21 + i, (0, 1)) for i, p in enumerate(clouds)]
    for early in (1, 0):
        old = capi.set_config(list_mask=1, mask_early=early)
        try:
            out = [None] * len(clouds)
            errs = []

            def run(i):
                try:
                    with capi.Cloud(clouds[i]) as c:
                        for _ in range(3):
                            r = _result(c.fit(0, 0.01, 3000, 1.0, seed=21 + i))
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
        finally:
            capi.restore_config(old)
