"""The PPF model preprocessing on the GPU.  m3d_orient_normals_mst (Boruvka over the cell-sorted grid) against the restatement's
heap walk (tests/cpp/ppf_train_ref.c): parent and the output normals byte for byte, stats equal, on every family of
ppf_train_ref_util -- tests/test_ppf_train.py holds the restatement to an independent Kruskal on the same inputs.
m3d_ppf_prepare_model against the restatement composed with the library's own estimate_normals and detect_boundary_points."""
import math

import numpy as np
import pytest

import ppf_edge_ref_util as eu
import ppf_train_ref_util as tu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tu.TrainRef(tmp_path_factory.mktemp("ppf_train_ref"))


def _same(got, want):
    (gn, gp, gs), (wn, wp, ws) = got, want
    assert np.array_equal(gp, wp)
    assert gn.tobytes() == wn.tobytes()
    assert {k: gs[k] for k in tu.STATS} == ws


@pytest.mark.parametrize("name", tu.ORIENT_CASES)
def test_orient_equals_the_heap_walk(capi, ref, name):
    c = tu.orient_case(name)
    got = capi.orient_normals_mst(**c)
    want = ref.orient(**c)
    _same(got, want)
    n, st = len(c["points"]), got[2]
    assert 1 <= st["rounds"] <= math.ceil(math.log2(max(n, 2))) + 1
    if name == "path":
        assert st["rounds"] >= 2 and st["component"] == n
    if name == "lattice":
        assert st["tree_edges"] == n - 1
    if name == "two_clusters":
        assert (got[1][150:] == -2).all() and got[0][150:].tobytes() == c["normals"][150:].tobytes() and st["component"] == 150
    if name == "on_radius":
        assert got[1][0] == -2 and st["tree_edges"] == 2
    if name == "sphere":
        centre = np.array([0.3, -0.2, 0.1])
        assert st["component"] == n and (((c["points"] - centre) * got[0]).sum(axis=1) > 0).all()


def test_orient_does_not_depend_on_scratch(capi, ref):
    c = tu.orient_case("sphere")
    want = capi.orient_normals_mst(**c)
    with capi.scratch_fill(0xFF):
        filled = capi.orient_normals_mst(**c)
    big = tu.sphere_case(50000, seed=9)
    capi.orient_normals_mst(**big)                 # ten times the size on the same lane: its blocks come back to the small call
    after = capi.orient_normals_mst(**c)
    for got in (filled, after):
        assert np.array_equal(got[1], want[1]) and got[0].tobytes() == want[0].tobytes()
        assert {k: got[2][k] for k in tu.STATS} == {k: want[2][k] for k in tu.STATS}


def test_orient_errors(capi):
    c = tu.orient_case("random_255")
    bad = c["points"].copy()
    bad[17, 1] = np.nan
    with pytest.raises(capi.M3DError, match="point 17 is not finite"):
        capi.orient_normals_mst(bad, c["normals"], c["radius"], c["seed"])
    for radius in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(capi.M3DError, match="radius"):
            capi.orient_normals_mst(c["points"], c["normals"], radius, c["seed"])
    with pytest.raises(capi.M3DError, match="seed"):
        capi.orient_normals_mst(c["points"], c["normals"], c["radius"], 255)
    L = capi.lib()
    assert L.m3d_orient_normals_mst(None, None, 4, 1.0, 0, 0, None, None, None) == -5
    import misc3d_amd as m3d
    got = m3d.pose_estimation.orient_normals(c["points"], c["normals"], c["radius"], c["seed"])
    want = capi.orient_normals_mst(**c)
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])


# ---- m3d_ppf_prepare_model
@pytest.fixture(scope="module")
def clouds():
    pts, nrm, _, _, _ = eu.plate_with_holes(n_side=84, seed=11)
    rng = np.random.default_rng(12)
    pts = pts + np.array([0.1, -0.2, 1.5]) + rng.normal(0, 0.002, size=pts.shape)
    nrm = nrm * rng.choice([-1.0, 1.0], size=(len(nrm), 1)) * rng.uniform(0.5, 2.0, size=(len(nrm), 1))
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raycast_obj.npz"))
    obj = np.ascontiguousarray(g["vertices"].astype(np.float64) * 0.001)
    return dict(plate=(np.ascontiguousarray(pts), np.ascontiguousarray(nrm)), obj=(obj, None))


def _composed(capi, ref, pts, nrm, dense, box=None, keep=False, **params):
    """the restatement's host steps around the library's own two device calls"""
    c, e = ref.box(pts) if box is None else box
    d = ref.derive(c, e, params.get("rel_sample_dist", 0.05), params.get("rel_dense_sample_dist", 0.025), params.get("calc_normal_relative", 0.01))
    given = nrm is not None
    n0 = nrm if given else capi.estimate_normals(pts, capi.SEARCH_HYBRID, d["normal_r"], 30)
    r = ref.prepare_model(pts, n0, box=(c, e), rel_dense_sample_dist=0.025 if dense else 0.0, keep_normals=keep and given,
                          **{k: v for k, v in params.items() if k != "rel_dense_sample_dist"})
    r["edge_indices"] = np.zeros(0, np.int64)
    if dense:
        di = r["dense_indices"]
        r["edge_indices"] = capi.detect_boundary_points(np.ascontiguousarray(pts[di]), np.ascontiguousarray(r["normals"][di]), capi.SEARCH_HYBRID,
                                                        d["normal_r"], params.get("pts_num", 20), 90.0).astype(np.int64)
    return r


def _check_model(got, want):
    assert got["normals"].tobytes() == want["normals"].tobytes()
    for k in ("sample_indices", "dense_indices", "edge_indices"):
        assert np.array_equal(got[k], want[k]), k
    gi, wi = got["info"], want["info"]
    for k in ("diameter", "r_min", "dist_step", "dist_step_dense", "normal_r", "seed", "seed_flipped", "oriented"):
        assert gi[k] == wi[k], k
    for k in ("box_center", "box_extent", "view_pt"):
        assert np.array_equal(gi[k], wi[k]), k
    if wi["oriented"]:
        assert {k: gi["orient"][k] for k in tu.STATS} == wi["orient"]


@pytest.mark.parametrize("dense", (False, True), ids=("sample_only", "with_edges"))
@pytest.mark.parametrize("which,given", (("plate", True), ("plate", False), ("obj", False)), ids=("plate_given", "plate_estimated", "obj_estimated"))
def test_prepare_model_equals_the_composed_restatement(capi, ref, clouds, which, given, dense):
    pts, nrm = clouds[which]
    nrm = nrm if given else None
    # (the plate is thin: a normal radius of 3 % of its diameter holds enough points for a plane fit)
    params = dict(calc_normal_relative=0.03) if which == "plate" else {}
    got = capi.ppf_prepare_model(pts, nrm, rel_dense_sample_dist=0.025 if dense else 0.0, **params)
    want = _composed(capi, ref, pts, nrm, dense, **params)
    _check_model(got, want)
    assert 50 < len(got["sample_indices"]) < len(pts) and len(set(got["sample_indices"].tolist())) == len(got["sample_indices"])
    if dense:
        # (the plate has rims and holes; the object is a closed surface and may have no edge point at all)
        assert len(got["dense_indices"]) > len(got["sample_indices"]) and len(got["edge_indices"]) < len(got["dense_indices"])
        assert which != "plate" or len(got["edge_indices"]) > 0
    else:
        assert len(got["dense_indices"]) == 0 and len(got["edge_indices"]) == 0


def test_prepare_model_with_a_callers_box_and_external_normals(capi, ref, clouds):
    pts, nrm = clouds["plate"]
    box = (np.array([0.12, -0.18, 1.49]), np.array([1.05, 0.8, 0.02]))
    got = capi.ppf_prepare_model(pts, nrm, box_center=box[0], box_extent=box[1], calc_normal_relative=0.03)
    _check_model(got, _composed(capi, ref, pts, nrm, True, box=box, calc_normal_relative=0.03))
    assert np.array_equal(got["info"]["box_extent"], box[1])
    ext = capi.ppf_prepare_model(pts, nrm, use_external_normal=1, calc_normal_relative=0.03)
    _check_model(ext, _composed(capi, ref, pts, nrm, True, keep=True, calc_normal_relative=0.03))
    assert ext["info"]["oriented"] == 0
    s = (nrm * nrm).sum(axis=1)
    assert np.abs(np.linalg.norm(ext["normals"], axis=1) - 1).max() < 1e-12 and (np.sign((ext["normals"] * nrm).sum(axis=1)) > 0).all() and (s > 0).all()
    inv = capi.ppf_prepare_model(pts, nrm, invert_model_normal=1, calc_normal_relative=0.03)
    _check_model(inv, _composed(capi, ref, pts, nrm, True, invert_model_normal=True, calc_normal_relative=0.03))
    i = inv["info"]
    assert i["seed_flipped"] == 1 - int(np.dot(i["view_pt"] - pts[i["seed"]], nrm[i["seed"]]) < 0)
    with pytest.raises(capi.M3DError, match="There is no input points"):
        capi.ppf_prepare_model(np.zeros((0, 3)))
