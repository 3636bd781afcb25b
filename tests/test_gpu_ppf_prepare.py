"""m3d_ppf_prepare_scene (PPFEstimator::PreprocessEstimate) on the GPU: bit for bit the same sequence made of the library's
public calls -- estimate_normals, voxel_down_sample, detect_boundary_points -- with a numpy restatement of the two host steps in
between (the non-finite rows dropped, NormalConsistent)."""
import numpy as np
import pytest

import ppf_edge_ref_util as eu

pytestmark = pytest.mark.gpu

DIAMETER, NORMAL_R, STEP, STEP_DENSE, PTS_NUM = 1.22, 0.05, 0.05, 0.02, 30


@pytest.fixture(scope="module")
def cloud():
    """the plate with holes sampled by a few thousand points, in front of the origin, with 37 rows made non-finite -> (points, unit normals
    of mixed sign)"""
    pts, nrm, _, _, _ = eu.plate_with_holes(n_side=84, seed=11)
    rng = np.random.default_rng(12)
    pts = pts + np.array([0.1, -0.2, 1.5]) + rng.normal(0, 0.002, size=pts.shape)
    nrm = nrm * rng.choice([-1.0, 1.0], size=(len(nrm), 1)) * rng.uniform(0.5, 2.0, size=(len(nrm), 1))      # any sign, any length
    bad = rng.choice(len(pts), size=37, replace=False)
    pts[bad[:20], rng.integers(0, 3, size=20)] = np.nan
    pts[bad[20:30], rng.integers(0, 3, size=10)] = np.inf
    pts[bad[30:], rng.integers(0, 3, size=7)] = -np.inf
    return np.ascontiguousarray(pts), np.ascontiguousarray(nrm)


def _normal_consistent(p, n):
    """NormalConsistent (include/misc3d/utils.h:130-144) in numpy: the same rounded operations in the same order"""
    n = n.copy()
    flip = (p[:, 0] * n[:, 0] + p[:, 1] * n[:, 1]) + p[:, 2] * n[:, 2] > 0.0
    n[flip] = -n[flip]
    s = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    ok = s > 0.0
    n[ok] = n[ok] / np.sqrt(s[ok])[:, None]
    return n


def _composed(capi, pts, nrm, dense):
    keep = np.isfinite(pts).all(axis=1)
    p = np.ascontiguousarray(pts[keep])
    n = np.ascontiguousarray(nrm[keep]) if nrm is not None else capi.estimate_normals(p, capi.SEARCH_HYBRID, NORMAL_R * DIAMETER, 30)
    n = _normal_consistent(p, n)
    s = capi.voxel_down_sample(p, STEP, normals=n)
    out = dict(sample_points=s["points"], sample_normals=s["normals"], dense_points=np.zeros((0, 3)), dense_normals=np.zeros((0, 3)),
               edge_indices=np.zeros(0, np.int64))
    if dense:
        d = capi.voxel_down_sample(p, STEP_DENSE, normals=n)
        out.update(dense_points=d["points"], dense_normals=d["normals"],
                   edge_indices=capi.detect_boundary_points(d["points"], d["normals"], capi.SEARCH_HYBRID, NORMAL_R * DIAMETER, PTS_NUM, 90.0))
    return out


@pytest.mark.parametrize("dense", (False, True), ids=("sample_only", "with_edges"))
@pytest.mark.parametrize("with_normals", (True, False), ids=("given_normals", "estimated_normals"))
def test_prepare_scene_equals_the_composed_calls(capi, cloud, with_normals, dense):
    pts, nrm = cloud
    nrm = nrm if with_normals else None
    got = capi.ppf_prepare_scene(pts, nrm, DIAMETER, NORMAL_R, STEP, STEP_DENSE if dense else 0.0, PTS_NUM)
    want = _composed(capi, pts, nrm, dense)
    for k in ("sample_points", "sample_normals", "dense_points", "dense_normals"):
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
    assert np.array_equal(got["edge_indices"], want["edge_indices"].astype(np.int64))
    assert 100 < len(got["sample_points"]) < len(pts) - 37
    if dense:
        e = got["edge_indices"]
        assert len(got["dense_points"]) > len(got["sample_points"]) and 0 < len(e) < len(got["dense_points"])
        assert (np.diff(e) > 0).all()
        assert np.array_equal(e, capi.detect_boundary_points(got["dense_points"], got["dense_normals"], capi.SEARCH_HYBRID,
                                                             NORMAL_R * DIAMETER, PTS_NUM, 90.0).astype(np.int64))
    else:
        assert len(got["dense_points"]) == 0 and len(got["edge_indices"]) == 0


def test_python_entry_and_errors(capi, cloud):
    import misc3d_amd as m3d
    pts, nrm = cloud
    r = m3d.pose_estimation.ppf_prepare_scene(pts, nrm, DIAMETER, NORMAL_R, STEP, STEP_DENSE, PTS_NUM)
    want = capi.ppf_prepare_scene(pts, nrm, DIAMETER, NORMAL_R, STEP, STEP_DENSE, PTS_NUM)
    assert all(np.array_equal(r[k], want[k]) for k in want)
    with pytest.raises(RuntimeError, match="voxel_size"):
        m3d.pose_estimation.ppf_prepare_scene(pts, nrm, DIAMETER, NORMAL_R, 0.0)          # the composed call's own error
    with pytest.raises(RuntimeError, match="There is no scene point clouds."):
        m3d.pose_estimation.ppf_prepare_scene(np.zeros((0, 3)), None, DIAMETER, NORMAL_R, STEP)
