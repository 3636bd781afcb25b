"""misc3d.segmentation.ProximityExtractor, no GPU needed: the plain-C restatement of the reference's serial Segment
(tests/cpp/proximity_ref.c) equals the connected components of the accepted radius graph (the equivalence the device
union-find rests on), the host cut-offs (m3d_proximity_fp.hpp, through m3d_bench_proximity_cutoffs) equal the direct
sqrt / acos tests, and the new symbols are exported."""
import ctypes as C

import numpy as np
import pytest

from proximity_ref_util import build_ref, canonical, scipy_partition


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("prox_ref"))


def test_symbols_exported():
    from misc3d_amd import capi
    L = C.CDLL(capi.LIB_PATH)
    for name in ("m3d_proximity_segment", "m3d_proximity_segment_nn", "m3d_radius_neighbors",
                 "m3d_bench_proximity_cutoffs"):
        assert hasattr(L, name), name
    import misc3d_amd as m3d
    for name in ("ProximityExtractor", "BaseProximityEvaluator", "DistanceProximityEvaluator",
                 "NormalsProximityEvaluator", "DistanceNormalsProximityEvaluator"):
        assert hasattr(m3d.segmentation, name), name


@pytest.mark.parametrize("seed", range(4))
def test_restatement_is_the_component_partition(ref, seed):
    rng = np.random.default_rng(seed)
    n = 3000
    xyz = rng.uniform(0, 1, (n, 3))
    xyz[rng.integers(0, n, 200)] = xyz[rng.integers(0, n, 200)]   # duplicates
    xyz[rng.integers(0, n, 5), 1] = np.nan
    for r, t in ((0.05, 0.04), (0.08, 1.0), (0.03, 0.03)):
        cl, lab = ref.segment(xyz, r, "distance", dist=t)
        assert cl == scipy_partition(xyz, r, dist=t), (seed, r, t)
        for k, c in enumerate(cl):
            assert (lab[c] == k).all()


def test_restatement_normals_partition(ref):
    """Normals / DistanceNormals: components of the pairs whose evaluator accepts (the evaluator is symmetric)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(7)
    n = 2000
    xyz = rng.uniform(0, 1, (n, 3))
    nrm = rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    for kind, dist, ang in (("normals", 0.0, 40.0), ("distance_normals", 0.05, 60.0), ("distance_normals", 0.07, -50.0)):
        cl, _ = ref.segment(xyz, 0.07, kind, dist=dist, angle=ang, normals=nrm)
        p = cKDTree(xyz).query_pairs(0.07 * 1.0001, output_type="ndarray")
        a, b = p[:, 0], p[:, 1]
        d = xyz[a] - xyz[b]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        dot = (nrm[a, 0] * nrm[b, 0] + nrm[a, 1] * nrm[b, 1]) + nrm[a, 2] * nrm[b, 2]
        keep = (d2 <= 0.07 * 0.07) & ref.angle_test(dot, ang)
        if kind == "distance_normals":
            keep &= ref.dist_test(d2, dist, True)
        g = coo_matrix((np.ones(keep.sum()), (a[keep], b[keep])), shape=(n, n))
        assert cl == canonical(connected_components(g, directed=False)[1]), kind


def test_restatement_min_max_and_nn_overload(ref):
    xyz = np.array([[0, 0, 0], [0.1, 0, 0], [0.2, 0, 0], [5, 5, 5], [5.1, 5, 5], [9, 9, 9]], float)
    cl, lab = ref.segment(xyz, 0.15, "distance", dist=1.0)
    assert cl == [[0, 1, 2], [3, 4], [5]] and lab.tolist() == [0, 0, 0, 1, 1, 2]
    cl, lab = ref.segment(xyz, 0.15, "distance", dist=1.0, min_size=2, max_size=2)
    assert cl == [[3, 4]] and lab.tolist() == [1, 1, 1, 0, 0, 1]
    cl, _ = ref.segment_nn(xyz, [[0, 1], [1], [2, 1], [3], [4, 3], [5]], "distance", dist=1.0)
    assert cl == [[0, 1, 2], [3, 4], [5]]


def _cut_cases():
    return [0.0, -0.0, 30.0, -30.0, 90.0, 180.0, 200.0, float("nan"), -90.0, -180.0, 1e-7, 179.9]


def test_distance_cutoffs_equal_sqrt(ref):
    from misc3d_amd import capi
    rng = np.random.default_rng(1)
    for t in (0.02, 1.0, 1e-150, 3e150, 0.0, -1.0, np.inf, np.nan, 0.7071067811865476):
        c = capi.proximity_cutoffs(t, 0.0)[0]
        base = abs(t) if np.isfinite(t) and t != 0 else 1.0
        near = [np.nextafter(c, -np.inf), np.nextafter(c, np.inf)] if np.isfinite(c) else []
        d2 = np.concatenate([rng.uniform(0, 2, 1_000_000) * base * base, [0.0, np.inf, np.nan, c], near])
        d2 = d2[~(d2 < 0)]
        with np.errstate(invalid="ignore"):
            assert np.array_equal(d2 < c, ref.dist_test(d2, t, False)), t
            assert np.array_equal(~(d2 >= c), ref.dist_test(d2, t, True)), t


@pytest.mark.parametrize("ang", _cut_cases())
def test_angle_cutoffs_equal_acos(ref, ang):
    from misc3d_amd import capi
    _, lo1, hi1, lo2, hi2 = capi.proximity_cutoffs(0.0, ang)
    rng = np.random.default_rng(2)
    ends = [v for v in (lo1, hi1, lo2, hi2) if np.isfinite(v)]
    near = [np.nextafter(v, s) for v in ends for s in (-np.inf, np.inf)]
    dot = np.concatenate([rng.uniform(-1.0000001, 1.0000001, 1_000_000), rng.uniform(0.999, 1.000001, 100_000),
                          rng.uniform(-1.000001, -0.999, 100_000), ends, near,
                          [1.0, -1.0, np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), 0.0, -0.0, np.nan, np.inf, 1.5]])
    with np.errstate(invalid="ignore"):
        got = ((dot >= lo1) & (dot <= hi1)) | ((dot >= lo2) & (dot <= hi2))
    assert np.array_equal(got, ref.angle_test(dot, ang))
