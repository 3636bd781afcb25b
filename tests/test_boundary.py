"""DetectBoundaryPoints without a GPU: the independent reference (tests/boundary_ref_util.py) against hand-computed cases,
and the C oracle against the reference on every input family the GPU tests use.  Per family the two CONDITIONS the GPU
tests rely on are asserted here, for the reference alone: no point's gap within the margin of the threshold, and
conditioning >= 1e-6 for every point with at least 3 neighbours."""
import numpy as np
import pytest

import boundary_ref_util as bru
from boundary_ref_util import HYBRID, KNN, RADIUS


@pytest.fixture(scope="module")
def eigvec(orc):
    return orc.j3x3_smallest_eigvec


def _ref(eigvec, pts, nrm, search, radius, max_nn, thr=90.0):
    return bru.reference(np.asarray(pts, np.float64), nrm, search, radius, max_nn, thr, eigvec)


def test_reference_star(eigvec):
    """centre + neighbours at 0, 90, 180 and 225 degrees in z = 0: gaps 90, 90, 45, 135 -> the centre's gap is 135 degrees;
    each arm sees the others within a half plane or less"""
    arms = np.radians([0.0, 90.0, 180.0, 225.0])
    pts = np.r_[[[0.0, 0.0, 0.0]], np.c_[np.cos(arms), np.sin(arms), np.zeros(4)]]
    nrm = np.tile([0.0, 0.0, 1.0], (5, 1))
    for normals in (nrm, -nrm, 2.5 * nrm):
        r = _ref(eigvec, pts, normals, RADIUS, 10.0, 0, 134.0)
        assert r.m.tolist() == [5] * 5 and r.na.tolist() == [4] * 5
        assert abs(np.degrees(r.gap[0]) - 135.0) < 1e-12 and r.flag[0]
        assert not _ref(eigvec, pts, normals, RADIUS, 10.0, 0, 136.0).flag[0]
        # arm at 0 degrees, (1, 0): the others lie at directions 135 (to (0, 1)), 180 and 180 + atan(1 / (1 + sqrt 2)) = 202.5
        assert abs(np.degrees(r.gap[1]) - (360.0 - 67.5)) < 1e-12
        assert np.all(r.cond > 1 - 1e-15)
    # the three nearest of the centre (itself, then the arms by index on the tie): arms at 0 and 90 -> gap 270
    r = _ref(eigvec, pts, nrm, KNN, 0.0, 3)
    assert r.nb[0].tolist() == [0, 1, 2] and abs(np.degrees(r.gap[0]) - 270.0) < 1e-12
    # without normals: the plane's own normal, same gaps
    r = _ref(eigvec, pts, None, RADIUS, 10.0, 0, 134.0)
    assert abs(np.degrees(r.gap[0]) - 135.0) < 1e-9


def test_reference_square_lattice(eigvec):
    g = np.stack(np.meshgrid(np.arange(6.0), np.arange(6.0), indexing="ij"), -1).reshape(-1, 2)
    pts = np.c_[g, np.zeros(36)]
    nrm = np.tile([0.0, 0.0, 1.0], (36, 1))
    r = _ref(eigvec, pts, nrm, RADIUS, 1.0, 0)                       # d2 <= 1: the four axis neighbours
    on_edge = ((g == 0) | (g == 5)).sum(axis=1)
    assert np.allclose(np.degrees(r.gap[on_edge == 0]), 90.0, atol=1e-12) and (r.m[on_edge == 0] == 5).all()
    assert np.allclose(np.degrees(r.gap[on_edge == 1]), 180.0, atol=1e-12) and (r.m[on_edge == 1] == 4).all()
    assert np.allclose(np.degrees(r.gap[on_edge == 2]), 270.0, atol=1e-12) and (r.m[on_edge == 2] == 3).all()
    assert r.flag[on_edge > 0].all()
    assert bru.compare(on_edge > 0, r) == 36 - 20                   # the interior sits ON the threshold: undecided
    assert np.array_equal(_ref(eigvec, pts, nrm, RADIUS, 1.0, 0, 91.0).flag, on_edge > 0)
    h = _ref(eigvec, pts, nrm, HYBRID, 1.0, 30)                      # d2 < 1: nobody but the point itself
    assert (h.m == 1).all() and not h.flag.any() and np.isnan(h.gap).all()
    with pytest.raises(AssertionError):
        bru.compare(~r.flag, r)
    assert bru.compare(np.flatnonzero(on_edge > 0), r) == 16         # index form


def test_reference_nonfinite_rules(eigvec):
    rng = np.random.default_rng(1)
    pts = rng.uniform(0, 1, (40, 3))
    pts[:, 2] *= 0.01
    clean = _ref(eigvec, pts[5:], None, KNN, 0.0, 8)
    for bad in (np.nan, np.inf, -np.inf):
        p = pts.copy()
        p[0] = bad
        p[1, 0] = p[2, 1] = p[3, 2] = bad
        p[4, :2] = bad
        for search, radius, k in ((KNN, 0.0, 8), (RADIUS, 0.4, 0), (HYBRID, 0.4, 8)):
            r = _ref(eigvec, p, None, search, radius, k)
            assert (r.m[:5] == 0).all() and not r.flag[:5].any() and np.isnan(r.gap[:5]).all()
            assert (r.nb >= 5).sum() == (r.nb >= 0).sum()           # nobody's neighbour
        r = _ref(eigvec, p, None, KNN, 0.0, 8)                      # = the cloud without them, indices shifted by 5
        assert np.array_equal(r.flag[5:], clean.flag) and np.array_equal(r.gap[5:], clean.gap)
        assert np.array_equal(r.nb[5:], clean.nb + 5)
    two = pts[:6].copy()
    two[2:] = np.nan                                                 # fewer than 3 neighbours: not flagged
    assert not _ref(eigvec, two, None, KNN, 0.0, 5).flag.any()
    nrm = np.tile([0.0, 0.0, 1.0], (40, 1))
    nrm[7], nrm[8], nrm[9, 0] = 0.0, np.nan, np.nan                  # no direction: not flagged, whatever the threshold
    r = _ref(eigvec, pts, nrm, KNN, 0.0, 8, -5.0)
    assert not r.flag[7:10].any() and r.flag[10:].all()


def test_reference_neighbour_order(eigvec):
    """(d2, index) order and the Radius / Hybrid rule at d2 == r*r, on exact distances"""
    pts = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -2, 0], [1, 0, 0], [0, 0, 0]], np.float64)
    nb, m = bru.neighbourhoods(pts, RADIUS, 2.0, 0)
    assert nb[0, :m[0]].tolist() == [0, 6, 2, 3, 5, 1, 4]
    nb, m = bru.neighbourhoods(pts, HYBRID, 2.0, 128)
    assert nb[0, :m[0]].tolist() == [0, 6, 2, 3, 5]
    nb, m = bru.neighbourhoods(pts, HYBRID, 2.0, 4)
    assert nb[0, :m[0]].tolist() == [0, 6, 2, 3]
    nb, m = bru.neighbourhoods(pts, KNN, 0.0, 6)
    assert nb[0, :m[0]].tolist() == [0, 6, 2, 3, 5, 1]


@pytest.mark.parametrize("name", list(bru.CASES))
def test_family_conditions_and_oracle(orc, eigvec, name):
    case = bru.CASES[name]()
    ref = case.reference(eigvec)
    assert len(case.pts) <= 4000
    undecided = int((np.abs(ref.gap - ref.thr_rad) < bru.MARGIN).sum())
    cond = ref.cond[ref.m >= 3]
    print(f"{name}: n {len(case.pts)}, flagged {int(ref.flag.sum())}, undecided {undecided}, "
          f"min conditioning {cond.min() if len(cond) else np.inf:.3g}")
    assert undecided == 0
    assert (cond >= bru.MIN_CONDITIONING).all()
    if case.oracle:
        assert bru.compare(orc.detect_boundary_points(*case.args()), ref) == 0


def test_family_properties(eigvec):
    """what the GPU tests assume about their inputs, from the reference"""
    nb_h, m_h = bru.neighbourhoods(bru.seam_cloud()[0], HYBRID, bru.SEAM_RADIUS, 128)
    nb_r, m_r = bru.neighbourhoods(bru.seam_cloud()[0], RADIUS, bru.SEAM_RADIUS, 0)
    assert m_h.max() == 32 and np.array_equal(m_h, m_r)              # <= 32 strictly inside, none at d2 == r*r
    assert (m_h >= 31).sum() > 50                                     # and the 31 | 32 | 33 cuts do cut
    _, m = bru.neighbourhoods(bru.radius_cap_cloud(128), RADIUS, bru.RADIUS_CAP_R, 0)
    assert m.max() == 128 and (m == 128).sum() == 128
    _, m = bru.neighbourhoods(bru.radius_cap_cloud(129), RADIUS, bru.RADIUS_CAP_R, 0)
    assert m.max() == 129
    p, _ = bru.duplicates_cloud()
    r = bru.CASES["duplicates-knn-normals"]().reference(eigvec)
    rep = np.flatnonzero((p == p[np.argmax((r.m >= 3) & (r.na == 0))]).all(axis=1))
    assert len(rep) == 40 and (r.na[rep] == 0).all() and not r.flag[rep].any()
    lat = bru.CASES["ties-radius-100"]().reference(eigvec)
    assert lat.m.max() == 13                                          # d2 = 4 included: 1 + 4 + 4 + 4
    assert bru.CASES["ties-hybrid-all-100"]().reference(eigvec).m.max() == 9
    unit = bru.CASES["ties-radius-unit-100"]().reference(eigvec)       # the ring ON the radius decides: the lattice's rim
    assert unit.m.max() == 5 and unit.flag.sum() == 4 * 30 - 4
    assert bru.CASES["ties-radius-unit-200"]().reference(eigvec).flag.sum() == 4
    assert bru.CASES["ties-hybrid-unit-100"]().reference(eigvec).m.max() == 1
