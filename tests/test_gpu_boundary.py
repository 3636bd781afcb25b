"""DetectBoundaryPoints on the GPU against the oracle: identical index sets, with given
normals and with normals estimated from the neighbourhood, for Hybrid and Radius searches; API checks.  Further down: both
kernel bodies at their seams, judged by the independent reference of tests/boundary_ref_util.py."""
import numpy as np
import pytest

import boundary_ref_util as bru

pytestmark = pytest.mark.gpu


def _patch(n, seed, holes=True):
    rng = np.random.default_rng(seed)
    uv = rng.uniform(0, 1, (n, 2))
    if holes:                                            # a disc cut out of the patch: inner boundary too
        uv = uv[np.hypot(uv[:, 0] - 0.5, uv[:, 1] - 0.5) > 0.18]
    pts = np.c_[uv[:, 0], uv[:, 1], 0.3 * uv[:, 0] - 0.2 * uv[:, 1] + rng.normal(0, 1e-4, len(uv))]
    nrm = np.tile(np.array([-0.3, 0.2, 1.0]) / np.linalg.norm([-0.3, 0.2, 1.0]), (len(uv), 1))
    return np.ascontiguousarray(pts), nrm, uv


@pytest.mark.parametrize("search,radius,max_nn", [(2, 0.05, 30), (2, 0.08, 12), (2, 0.03, 128), (1, 0.04, 0),
                                                  (0, 0.0, 30), (0, 0.0, 7), (0, 0.0, 128)])
@pytest.mark.parametrize("with_normals", [True, False])
def test_boundary_matches_oracle(capi, orc, search, radius, max_nn, with_normals):
    pts, nrm, uv = _patch(3500, seed=int(radius * 1000) + max_nn)
    pts[[5, 99]] = pts[7]                                # coincident points (skipped as neighbours, :36-38)
    n_in = nrm if with_normals else None
    got = capi.detect_boundary_points(pts, n_in, search, radius, max_nn, 90.0)
    ref = orc.detect_boundary_points(pts, n_in, search, radius, max_nn, 90.0)
    assert np.array_equal(got.astype(np.int64), ref)
    assert len(ref) > 50
    if radius >= 0.05 and max_nn >= 30:   # dense enough neighbourhoods: only real edges are flagged
        edge = np.minimum.reduce([uv[:, 0], 1 - uv[:, 0], uv[:, 1], 1 - uv[:, 1],
                                  np.abs(np.hypot(uv[:, 0] - 0.5, uv[:, 1] - 0.5) - 0.18)])
        assert len(ref) < len(pts) // 2 and np.median(edge[ref]) < radius    # outer edge or the hole's rim


def test_boundary_threshold_and_errors(capi, orc):
    pts, nrm, _ = _patch(1500, seed=3, holes=False)
    for thr in (30.0, 120.0, 200.0):
        got = capi.detect_boundary_points(pts, nrm, 2, 0.07, 30, thr)
        assert np.array_equal(got.astype(np.int64), orc.detect_boundary_points(pts, nrm, 2, 0.07, 30, thr))
    far = pts * 50.0                                     # nobody has 3 neighbours within the radius
    assert len(capi.detect_boundary_points(far, None, 2, 0.05, 30, 90.0)) == 0
    with pytest.raises(capi.M3DError):
        capi.detect_boundary_points(pts[:0], None, 2, 0.05, 30, 90.0)      # "No PointCloud data."
    with pytest.raises(capi.M3DError):
        capi.detect_boundary_points(pts, None, 1, 0.5, 0, 90.0)            # radius search with > 128 neighbours
    with pytest.raises(capi.M3DError):
        capi.detect_boundary_points(pts, None, 0, 0.05, 200, 90.0)         # at most 128 neighbours
    few = pts[:20]                                                          # fewer points than k: all of them are used
    assert np.array_equal(capi.detect_boundary_points(few, None, 0, 0.0, 30, 90.0).astype(np.int64),
                          orc.detect_boundary_points(few, None, 0, 0.0, 30, 90.0))
    blob = np.ascontiguousarray(np.random.default_rng(4).normal(size=(2500, 3)))   # volume-filling cloud, KNN
    assert np.array_equal(capi.detect_boundary_points(blob, None, 0, 0.0, 20, 90.0).astype(np.int64),
                          orc.detect_boundary_points(blob, None, 0, 0.0, 20, 90.0))


def test_python_api_detect_boundary_points(capi):
    import misc3d_amd as m3d
    pts, nrm, _ = _patch(1200, seed=9)
    ref = capi.detect_boundary_points(pts, nrm, 2, 0.06, 30, 90.0).tolist()
    assert m3d.features.detect_boundary_points((pts, nrm), ("hybrid", 0.06, 30)) == ref

    class Param:                                          # duck-typed open3d.geometry.KDTreeSearchParamHybrid
        radius, max_nn = 0.06, 30

    class Cloud:
        points, normals = pts, nrm

    assert m3d.features.detect_boundary_points(Cloud(), Param()) == ref

    class Knn:                                            # duck-typed open3d.geometry.KDTreeSearchParamKNN
        knn = 25

    assert m3d.features.detect_boundary_points(Cloud(), Knn()) == capi.detect_boundary_points(pts, nrm, 0, 0.0, 25).tolist()
    assert m3d.features.detect_boundary_points(pts, ("knn", 25)) == capi.detect_boundary_points(pts, None, 0, 0.0, 25).tolist()


# ------------------------------------------------------------------------------------------------
# every kernel body at its seams, judged by the independent reference (tests/boundary_ref_util.py): each case of
# tests/test_boundary.py, where the reference alone is shown to leave no point undecided on these inputs
# ------------------------------------------------------------------------------------------------
def _got(capi, case):
    return capi.detect_boundary_points(*case.args()).astype(np.int64)


@pytest.mark.parametrize("name", list(bru.CASES))
def test_boundary_matches_reference(capi, orc, name):
    case = bru.CASES[name]()
    ref = case.reference(orc.j3x3_smallest_eigvec)
    got = _got(capi, case)
    assert np.array_equal(got, np.unique(got)) and (len(got) == 0 or got[-1] < len(case.pts))   # ascending, in range
    assert bru.compare(got, ref) == 0
    if case.oracle:
        assert np.array_equal(got, orc.detect_boundary_points(*case.args()))


def test_boundary_shell_hugs_the_rim(capi):
    pts, nrm = bru.shell()
    for scale in (1.0, -1.0, 0.5, 3.0):                  # the decision depends on the normal's direction only
        got = capi.detect_boundary_points(pts, scale * nrm, 2, 0.2, 30, 90.0).astype(np.int64)
        assert 50 < len(got) < len(pts) // 4 and np.median(bru.rim_distance(pts[got])) < 0.2


def test_boundary_unusable_normals_stay_unflagged(capi, orc):
    """a zero, NaN, infinite or overflowing normal gives no direction: never flagged, at 90 degrees and at a negative
    threshold, where every other point with a neighbour elsewhere is"""
    for name, n_bad in (("shell-zero-and-nan-normals", 7), ("shell-zero-and-nan-normals-threshold--10", 9)):
        case = bru.CASES[name]()
        bad = np.flatnonzero(~(np.isfinite(case.nrm).all(axis=1) & (case.nrm != 0).any(axis=1)) |
                             (np.abs(case.nrm) > 1e150).any(axis=1))
        assert len(bad) == n_bad
        ref = case.reference(orc.j3x3_smallest_eigvec)
        assert (ref.m[bad] >= 3).all() and (ref.na[bad] > 0).all() and not ref.flag[bad].any()
        got = _got(capi, case)
        assert not np.isin(bad, got).any()
        assert not np.isin(bad, orc.detect_boundary_points(*case.args())).any()
        if case.thr < 0:
            assert len(got) == int(((ref.m >= 3) & (ref.na > 0)).sum()) - n_bad > 700


@pytest.mark.parametrize("with_normals", [True, False])
def test_boundary_exact_symmetries(capi, orc, with_normals):
    """sign flips of any axis and the swap x <-> y leave every d2 = (dx^2 + dy^2) + dz^2 bit-identical: the neighbourhoods
    are the same and only the tangent basis differs, so the flagged set is the same outside the undecided points"""
    pts, nrm = bru.shell()
    base = bru.CASES["shell-hybrid" if with_normals else "shell-estimated"]()
    ref = base.reference(orc.j3x3_smallest_eigvec)
    assert bru.compare(_got(capi, base), ref) == 0
    for swap in (False, True):
        for sx in (1.0, -1.0):
            for sy in (1.0, -1.0):
                for sz in (1.0, -1.0):
                    f = lambda a: np.ascontiguousarray((a[:, [1, 0, 2]] if swap else a) * [sx, sy, sz])  # noqa: E731
                    got = capi.detect_boundary_points(f(pts), f(nrm) if with_normals else None, 2, 0.2, 30, 90.0)
                    assert bru.compare(got.astype(np.int64), ref) == 0, (swap, sx, sy, sz)


def test_boundary_lds_scratch_seam(capi):
    """<= 32 points strictly inside the radius and none on it (tests/test_boundary.py): Hybrid(32) runs the LDS body,
    Hybrid(33) and Radius the scratch body, over identical neighbourhoods"""
    pts, nrm = bru.seam_cloud()
    for n_in in (nrm, None):
        h32 = capi.detect_boundary_points(pts, n_in, 2, bru.SEAM_RADIUS, 32, 90.0)
        h33 = capi.detect_boundary_points(pts, n_in, 2, bru.SEAM_RADIUS, 33, 90.0)
        rad = capi.detect_boundary_points(pts, n_in, 1, bru.SEAM_RADIUS, 0, 90.0)
        assert len(h32) > 50 and np.array_equal(h32, h33) and np.array_equal(h32, rad)


def test_boundary_radius_cap(capi, orc):
    with pytest.raises(capi.M3DError, match="more than 128 neighbours"):
        capi.detect_boundary_points(bru.radius_cap_cloud(129), None, 1, bru.RADIUS_CAP_R, 0, 90.0)
    ok = bru.CASES["radius-cap-128"]()                   # and the library is fine afterwards; 128 is within the cap
    assert bru.compare(_got(capi, ok), ok.reference(orc.j3x3_smallest_eigvec)) == 0


def test_boundary_all_nonfinite_and_thresholds(capi, orc):
    for bad in (np.nan, np.inf, -np.inf):
        p = np.full((70, 3), bad)
        for search, radius, k in ((0, 0.0, 10), (1, 0.5, 0), (2, 0.5, 10)):
            assert len(capi.detect_boundary_points(p, None, search, radius, k, 90.0)) == 0
    p = np.random.default_rng(3).uniform(0, 1, (70, 3))
    p[::2, 1] = np.nan
    p[1::2, 0] = np.inf
    assert len(capi.detect_boundary_points(p, None, 0, 0.0, 10, 90.0)) == 0
    # threshold <= 0: everyone with >= 3 neighbours of which one at least is elsewhere; 361 degrees: nobody
    for thr in (0.0, -10.0):
        case = bru.CASES[f"threshold-{thr:.0f}"]()
        ref = case.reference(orc.j3x3_smallest_eigvec)
        want = np.flatnonzero((ref.m >= 3) & (ref.na > 0))
        assert 0 < len(want) < len(case.pts) and np.array_equal(_got(capi, case), want)
    assert len(_got(capi, bru.CASES["threshold-361"]())) == 0
