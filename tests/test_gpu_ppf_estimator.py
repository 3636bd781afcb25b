"""pose_estimation.PPFEstimator on the GPU, in the shape of the reference's examples/python/ppf_estimator.py built from what the
repository holds: trained on the vertices of tests/golden/raycast_obj.npz, the scene rendered by RayCastRenderer at the first
golden pose in front of a plane (ppf_estimator_scene_util builds both scenes; tests/test_ppf_train.py runs the restatement chain on
them without a GPU and finds it inside the same bar).  The class must return exactly what its stages return when they are called by hand, and its
top pose must lie within one dist_step / one angle_step of the rendering pose (the quantisation of the vote itself).  The same
in EdgePoints mode on the plate with holes of ppf_edge_ref_util."""
import numpy as np
import pytest

import ppf_estimator_scene_util as su

pytestmark = pytest.mark.gpu

def _config(m3d, normal_rel=su.OBJ_NORMAL_REL, **kw):
    c = m3d.pose_estimation.PPFEstimatorConfig()
    c.training_param.calc_normal_relative = normal_rel      # (why not the default: ppf_estimator_scene_util)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.fixture(scope="module")
def obj_scene():
    """-> (model points, scene points, the rendering pose): the mesh at its first golden pose in front of a plane"""
    import misc3d_amd as m3d
    meshes, poses, cam, T = su.obj_scene_meshes()
    r = m3d.pose_estimation.RayCastRenderer(cam)
    assert r.cast_rays(meshes, poses) is True
    pts, _ = r.get_point_cloud()
    assert pts.tobytes() == su.cloud_of(r.get_depth_map().numpy(), cam).tobytes()      # (the host's way to the same cloud)
    return np.ascontiguousarray(meshes[0][0]), np.ascontiguousarray(pts), T


_pose_error = su.pose_error


def _by_hand(m3d, capi, cfg, model, model_normals, scene, scene_normals, seed, edge):
    """the estimator's steps made by hand -> (results, the model info)"""
    tp, vp = cfg.training_param, cfg.voting_param
    m = capi.ppf_prepare_model(model, model_normals, rel_sample_dist=tp.rel_sample_dist, rel_dense_sample_dist=tp.rel_dense_sample_dist if edge else 0.0,
                               calc_normal_relative=tp.calc_normal_relative, pts_num=cfg.edge_param.pts_num)
    info, si = m["info"], m["sample_indices"]
    ekw = {}
    if edge:
        ei = m["dense_indices"][m["edge_indices"]]
        ekw = dict(edge_points=model[ei], edge_normals=m["normals"][ei])
    voting = m3d.pose_estimation.PPFVoting(model[si], m["normals"][si], info["diameter"], info["r_min"], rel_sample_dist=tp.rel_sample_dist,
                                           angle_step=vp.angle_step, min_dist_thresh=vp.min_dist_thresh, min_angle_thresh=vp.min_angle_thresh,
                                           faster_mode=vp.faster_mode, **ekw)
    s = capi.ppf_prepare_scene(scene, scene_normals, info["diameter"], tp.calc_normal_relative, info["dist_step"],
                               info["dist_step_dense"] if edge else 0.0, cfg.edge_param.pts_num)
    num = len(s["sample_points"])
    ref = capi.ppf_reference_indices(num, int(cfg.ref_param.ratio * num), seed)
    skw = dict(edge_points=s["dense_points"][s["edge_indices"]], edge_normals=s["dense_normals"][s["edge_indices"]]) if edge else {}
    res = voting.estimate(s["sample_points"], s["sample_normals"], ref, dist_threshold=cfg.rel_dist_thresh * info["diameter"],
                          angle_threshold=cfg.rel_angle_thresh, ratio=cfg.ref_param.ratio, score_thresh=cfg.score_thresh,
                          rel_dist_sparse_thresh=cfg.refine_param.rel_dist_sparse_thresh, num_result=cfg.num_result,
                          refine_method=cfg.refine_param.method.name, object_id=cfg.object_id, **skw)
    return res, info, s


def _same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.pose.tobytes() == y.pose.tobytes() and x.q.tobytes() == y.q.tobytes() and x.t.tobytes() == y.t.tobytes()
        assert (x.num_votes, x.score, x.object_id) == (y.num_votes, y.score, y.object_id)


def test_estimator_on_the_reference_examples_shape(capi, obj_scene):
    import misc3d_amd as m3d
    model, scene, T = obj_scene
    cfg = _config(m3d, score_thresh=0.01)               # (the example's)
    est = m3d.pose_estimation.PPFEstimator(cfg)
    assert est.estimate(scene) == (False, [])           # not trained yet
    assert est.train(model) is True
    d1 = est._dist_threshold
    assert est.train(model) is True and est._dist_threshold == d1 == cfg.rel_dist_thresh * est.get_model_diameter()
    ret, results = est.estimate(scene, seed=7)
    hand, info, s = _by_hand(m3d, capi, cfg, model, None, scene, None, 7, False)
    print("diameter", info["diameter"], "sample", len(est.get_sampled_model()[0]), "scene sample", len(s["sample_points"]), "results", len(results))
    assert ret is True and len(results) >= 1
    _same_results(results, hand)
    _same_results(est.get_pose(), results)
    dt, dr = _pose_error(results[0].pose, T)
    print("top pose: translation error", dt, "of dist_step", info["dist_step"], "rotation error", dr, "of angle_step", cfg.voting_param.angle_step,
          "votes", results[0].num_votes, "score", results[0].score)
    assert dt <= info["dist_step"] and dr <= cfg.voting_param.angle_step
    # the getters
    assert est.get_model_diameter() == info["diameter"]
    mp, mn = est.get_sampled_model()
    sp, sn = est.get_sampled_scene()
    assert mp.shape == mn.shape and mp.shape[1] == 3 and 50 < len(mp) < len(model)
    assert sp.tobytes() == s["sample_points"].tobytes() and sn.tobytes() == s["sample_normals"].tobytes()
    assert est.get_model_edges()[0].shape == (0, 3) and est.get_scene_edges()[0].shape == (0, 3)      # SampledPoints: no edge support
    # the config reaches the calls
    votes = [r.num_votes for r in results]
    assert votes == sorted(votes, reverse=True) and all(r.score >= 0.01 for r in results)
    one = m3d.pose_estimation.PPFEstimator(_config(m3d, score_thresh=0.01, num_result=1))
    assert one.train(model) is True
    ret1, res1 = one.estimate(scene, seed=7)
    assert ret1 is True and len(res1) == 1
    _same_results(res1, results[:1])
    strict = m3d.pose_estimation.PPFEstimator(_config(m3d, score_thresh=1.1))       # a score is min(1, ..): nothing passes
    assert strict.train(model) is True and strict.estimate(scene, seed=7) == (False, [])
    if len(results) > 1 and results[1].score < results[0].score:
        mid = 0.5 * (results[0].score + results[1].score)
        cut = m3d.pose_estimation.PPFEstimator(_config(m3d, score_thresh=mid))
        assert cut.train(model) is True
        _same_results(cut.estimate(scene, seed=7)[1], [r for r in results if r.score >= mid])
    assert isinstance(est.estimate(scene)[0], bool)     # a seed from the OS


def test_estimator_edge_points_mode(capi):
    import misc3d_amd as m3d
    model, nrm = su.plate_model()
    cfg = _config(m3d, su.PLATE_NORMAL_REL)
    cfg.voting_param.method = m3d.pose_estimation.PPFEstimatorConfig.EdgePoints
    est = m3d.pose_estimation.PPFEstimator(cfg)
    assert est.train(model, nrm) is True
    m = capi.ppf_prepare_model(model, nrm, calc_normal_relative=su.PLATE_NORMAL_REL, pts_num=cfg.edge_param.pts_num)
    sp, sn, T = su.plate_scene(model, m["normals"])
    ret, results = est.estimate(sp, sn, seed=7)
    hand, info, s = _by_hand(m3d, capi, cfg, model, nrm, sp, sn, 7, True)
    print("edge mode: model edges", len(est.get_model_edges()[0]), "scene edges", len(est.get_scene_edges()[0]), "results", len(results))
    assert ret is True and len(results) >= 1
    _same_results(results, hand)
    dt, dr = _pose_error(results[0].pose, T)
    print("edge mode top pose: translation error", dt, "of dist_step", info["dist_step"], "rotation error", dr, "of angle_step",
          cfg.voting_param.angle_step, "votes", results[0].num_votes, "score", results[0].score)
    assert dt <= info["dist_step"] and dr <= cfg.voting_param.angle_step
    ep, en = est.get_model_edges()
    ei = m["dense_indices"][m["edge_indices"]]
    assert ep.tobytes() == model[ei].tobytes() and en.tobytes() == m["normals"][ei].tobytes() and len(ep) > 0
    se, _ = est.get_scene_edges()
    assert se.tobytes() == s["dense_points"][s["edge_indices"]].tobytes() and len(se) > 0
