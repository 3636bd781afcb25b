"""PPF pose clustering on the GPU: m3d_ppf_cluster_poses against the contract's restatement (tests/cpp/ppf_cluster_ref.c), integer
for integer, on every input family of ppf_cluster_ref_util -- tests/test_ppf_cluster.py holds the restatement to the
numpy-longdouble judge and to the reference's stack on the same inputs, none of which has a pair near a threshold -- the
averaged poses against the judge; m3d_ppf_estimate end to end against the restatement with the ICP restatements for K7."""
import threading

import numpy as np
import pytest

import ppf_cluster_ref_util as cu

pytestmark = pytest.mark.gpu

POSE_BAR = 1e-12      # averaged poses against the judge: host arithmetic on both sides (the restatement is within 4e-15 of the
                      # judge on every family: DESIGN.md, "PPF pose clustering")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return cu.PcRef(tmp_path_factory.mktemp("ppf_cluster_ref"))


@pytest.fixture(scope="module")
def expected(ref):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ref.cluster(*cu.family(name))
        return cache[name]
    return get


def _cluster(capi, name, splits=0, **kw):
    capi.ppf_cluster_force(splits)
    try:
        return capi.ppf_cluster_poses(*cu.family(name), dist_threshold=cu.R_DIST, angle_threshold=cu.ANGLE, **kw)
    finally:
        capi.ppf_cluster_force(0)


def _assert_equal(got, want, judged=None):
    cu.assert_same_integers(got, want)
    assert got["stats"]["launches"] == (12 if want["stats"]["n_valid"] else 0)
    assert np.array_equal(got["avg_poses"], want["avg_poses"]) or np.abs(got["avg_poses"] - want["avg_poses"]).max() < POSE_BAR
    if judged is not None and len(judged["avg_poses"]):
        assert np.abs(got["avg_poses"] - judged["avg_poses"]).max() < POSE_BAR


@pytest.mark.parametrize("name", cu.FAMILIES)
def test_families(capi, expected, name):
    got = _cluster(capi, name)
    _assert_equal(got, expected(name), cu.judged(name))
    again = _cluster(capi, name)                      # the same call twice: nothing depends on scheduling
    cu.assert_same_integers(again, got)
    assert np.array_equal(again["avg_poses"], got["avg_poses"])


@pytest.mark.parametrize("splits", (1, 2, 3, 9))
@pytest.mark.parametrize("name", ("blobs_257", "blobs_2049", "chain", "bridge", "distinct_600"))
def test_workgroup_split_changes_nothing(capi, expected, name, splits):
    got = _cluster(capi, name, splits=splits)
    assert got["stats"]["splits"] == min(splits, (got["stats"]["n_valid"] + 255) // 256)
    _assert_equal(got, expected(name))


@pytest.mark.parametrize("name", cu.DISTINCT_VOTES)
def test_shuffled_input(capi, expected, name):
    """K1 breaks ties by input index, so a shuffled input gives equal results only where the votes are distinct: the families of
    DISTINCT_VOTES.  Positions are positions in the sorted list, which the shuffle leaves alone; `order` maps through it."""
    poses, votes = cu.family(name)
    perm = np.random.default_rng(17).permutation(len(votes))
    got = capi.ppf_cluster_poses(poses[perm], votes[perm], dist_threshold=cu.R_DIST, angle_threshold=cu.ANGLE)
    want = expected(name)
    assert np.array_equal(perm[got["order"]], want["order"])
    cu.assert_same_integers(dict(got, order=want["order"]), want)
    assert np.abs(got["avg_poses"] - want["avg_poses"]).max() < POSE_BAR


def test_four_threads_at_once(capi, expected):
    names = ("blobs_513", "chain", "blobs_2049", "split_rotation")
    out, errors = {}, []

    def run(name):
        try:
            out[name] = [_plain(capi, name) for _ in range(3)]
        except Exception as e:      # noqa: BLE001
            errors.append((name, e))

    def _plain(capi, name):
        return capi.ppf_cluster_poses(*cu.family(name), dist_threshold=cu.R_DIST, angle_threshold=cu.ANGLE)

    threads = [threading.Thread(target=run, args=(n,)) for n in names]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for name in names:
        for got in out[name]:
            _assert_equal(got, expected(name))


def test_python_class(capi, expected):
    import misc3d_amd as m3d
    import ppf_ref_util as pu

    pts, nrm, diameter, r_min = pu.model_case("box", 64)
    v = m3d.pose_estimation.PPFVoting(pts, nrm, diameter, r_min)
    poses, votes = cu.family("split_rotation")
    got = v.cluster_poses(poses, votes, dist_threshold=cu.R_DIST, angle_threshold=cu.ANGLE)
    _assert_equal(got, expected("split_rotation"))
    assert capi.ppf_cluster_params(v._model).dist_threshold == 0.05 * diameter


def test_capacity(capi, expected):
    want = expected("blobs_257")
    n, ct, cr = (want["stats"][k] for k in ("n_valid", "clusters_t", "clusters_r"))
    for kw in (dict(pose_capacity=n - 1, cluster_capacity=cr), dict(pose_capacity=n, cluster_capacity=cr - 1), dict(pose_capacity=0, cluster_capacity=0)):
        with pytest.raises(capi.M3DError) as e:
            _cluster(capi, "blobs_257", **kw)
        assert e.value.code == capi.ERR_CAPACITY and e.value.needed == (n, ct, cr)     # the needed counts
    _assert_equal(_cluster(capi, "blobs_257", pose_capacity=n, cluster_capacity=max(ct, cr)), want)
    # more valid poses than one call clusters: every pose valid (equal votes), far apart
    big = 262144 + 1
    poses = np.tile(np.eye(4), (big, 1, 1))
    poses[:, 0, 3] = np.arange(big)
    with pytest.raises(capi.M3DError) as e:
        capi.ppf_cluster_poses(poses, np.full(big, 3, np.uint32), dist_threshold=cu.R_DIST)
    assert e.value.code == capi.ERR_CAPACITY and e.value.needed[0] == big


# ---- m3d_ppf_estimate end to end
@pytest.fixture(scope="module")
def scene(capi):
    """ppf_ref_util's 1 200-point box model posed into clutter, its raw poses (the library's vote: tests/test_gpu_ppf.py holds it to
    its restatement) and what the restatement needs of the model"""
    return _scene_of(capi, cu.estimate_case())


def _scene_of(capi, c):
    model = capi.PpfModel(c["points"], c["normals"], c["diameter"], c["r_min"])
    raw = model.vote(c["scene_points"], c["scene_normals"], c["reference"])
    centred = c["points"] - model.centroid
    return dict(c, model=model, raw=raw, centred=np.ascontiguousarray(centred), dist_step=c["diameter"] * 0.05,
                dist_threshold=0.05 * c["diameter"])


@pytest.fixture(scope="module")
def icp(tmp_path_factory):
    import icp_ref_util as iu
    return iu.IcpRef(tmp_path_factory.mktemp("icp_ref"))


def _estimate(capi, s, **kw):
    kw.setdefault("angle_threshold", cu.ANGLE)
    return capi.ppf_estimate(s["model"], s["scene_points"], s["scene_normals"], s["reference"], **kw)


def _restated(ref, icp, s, **kw):
    return cu.estimate_ref(ref, icp, s["raw"]["poses"], s["raw"]["votes"], s["centred"], s["model"].centroid, s["scene_points"],
                           s["scene_normals"], s["dist_step"], s["dist_threshold"], **kw)


def _pose_err(A, B):
    return float(np.abs(np.asarray(A) - np.asarray(B)).max()) if len(A) else 0.0


# score_thresh = 0 where the list itself is under test: the reference scores against ratio x n^2 x 0.25 votes, which a scene of
# 300 reference points does not reach by far
@pytest.mark.parametrize("method", ("PointToPlane", "PointToPoint", "NoRefine"))
def test_estimate_against_the_restatement(capi, ref, icp, scene, method):
    got = _estimate(capi, scene, score_thresh=0.0, refine_method=method)
    want = _restated(ref, icp, scene, score_thresh=0.0, refine_method=method)
    print("%s: %d results, votes %s, scores %s, stats %s" % (method, len(got["votes"]), list(got["votes"]), list(got["scores"]), got["stats"]))
    print("pose differences to the restatement:", [_pose_err(a, b) for a, b in zip(got["poses"], want["poses"])])
    print("top pose to the truth:", _pose_err(got["poses"][0], scene["T"]) if len(got["poses"]) else None)
    assert len(got["votes"]) == len(want["votes"]) >= 1
    assert np.array_equal(got["votes"], want["votes"])
    assert np.array_equal(got["scores"], want["scores"])          # equal as doubles
    assert _pose_err(got["poses"], want["poses"]) < 1e-9
    assert _pose_err(got["t"], want["t"]) < 1e-9 and _pose_err(got["q"], want["q"]) < 1e-9
    assert np.array_equal(got["t"], got["poses"][:, :3, 3])
    if method == "NoRefine":
        # the shifted averaged poses: K6's output of m3d_ppf_cluster_poses, shifted by the centroid
        cl = capi.ppf_cluster_poses(scene["raw"]["poses"], scene["raw"]["votes"], dist_threshold=scene["dist_threshold"], angle_threshold=cu.ANGLE)
        shifted = ref.finish(cl["avg_poses"], cl["avg_votes"], scene["model"].centroid, 0.6, len(scene["centred"]), 0.0, 10 ** 6)
        for T, v in zip(got["poses"], got["votes"]):
            assert any(v == sv and np.array_equal(T, sT) for sT, sv in zip(shifted["poses"], shifted["votes"]))
        assert got["stats"]["icp_calls"] == 0
    else:
        assert got["stats"]["icp_calls"] == len(want["refined"])
    if method == "PointToPlane":
        assert _pose_err(got["poses"][0], scene["T"]) < 1e-9     # the top pose is the true pose
    # one vote, and the same one: the estimate runs the vote on the lane it holds, once
    assert got["stats"]["n_raw"] == len(scene["raw"]["votes"])
    assert got["stats"]["vote"]["launches"] == 1                 # (1 771 maxima: within the first launch's room for 4 096)


@pytest.mark.parametrize("method", ("PointToPlane", "PointToPoint"))
def test_estimate_two_instances(capi, ref, icp, method):
    """two copies of the model in one scene: two translation clusters, an ICP call each, results in vote order"""
    s = _scene_of(capi, cu.estimate_case_two())
    got = _estimate(capi, s, score_thresh=0.0, refine_method=method)
    want = _restated(ref, icp, s, score_thresh=0.0, refine_method=method)
    errs = [[_pose_err(T, truth) for truth in s["T"]] for T in got["poses"]]
    print("%s: votes %s, clusters %s, icp calls %d; differences to the restatement %s; to the two true poses %s"
          % (method, list(got["votes"]), got["stats"]["cluster"], got["stats"]["icp_calls"],
             [_pose_err(a, b) for a, b in zip(got["poses"], want["poses"])], errs))
    assert len(got["votes"]) == len(want["votes"]) >= 2 and got["stats"]["icp_calls"] == len(want["refined"]) >= 2
    assert np.array_equal(got["votes"], want["votes"]) and np.array_equal(got["scores"], want["scores"])
    assert list(got["votes"]) == sorted(got["votes"], reverse=True)
    assert _pose_err(got["poses"], want["poses"]) < 1e-9
    for k in range(2):                                   # each copy is found, at its true pose
        assert min(e[k] for e in errs) < 1e-9
    assert errs[0][0] < 1e-9                             # the copy voted at more reference points comes first


def test_two_threads_estimate_on_one_model(capi, scene):
    """two threads, three estimates each (default refinement) on one model: every result is the single-threaded call's"""
    want = _estimate(capi, scene, score_thresh=0.0)
    assert len(want["votes"]) >= 1 and want["stats"]["icp_calls"] >= 1
    results, errors = [[], []], []

    def work(slot):
        try:
            for _ in range(3):
                results[slot].append(_estimate(capi, scene, score_thresh=0.0))
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert [len(r) for r in results] == [3, 3]
    for got in results[0] + results[1]:
        assert np.array_equal(got["votes"], want["votes"]) and np.array_equal(got["scores"], want["scores"])
        assert _pose_err(got["poses"], want["poses"]) < 1e-9
        assert _pose_err(got["q"], want["q"]) < 1e-9 and _pose_err(got["t"], want["t"]) < 1e-9
        assert got["stats"]["n_raw"] == want["stats"]["n_raw"] and got["stats"]["vote"]["launches"] == want["stats"]["vote"]["launches"]


def test_estimate_cuts(capi, scene):
    full = _estimate(capi, scene, score_thresh=0.0, refine_method="NoRefine")
    top = float(full["scores"][0])
    assert 0.0 < top <= 1.0
    none = _estimate(capi, scene, score_thresh=min(1.5, top * 1.01 + 1e-6), refine_method="NoRefine")      # M3D_OK, no results
    assert len(none["votes"]) == 0 and none["poses"].shape == (0, 4, 4)
    one = _estimate(capi, scene, score_thresh=0.0, num_result=1, refine_method="NoRefine")
    assert len(one["votes"]) == 1 and np.array_equal(one["poses"][0], full["poses"][0])
    if len(full["votes"]) > 1:
        with pytest.raises(capi.M3DError) as e:
            _estimate(capi, scene, score_thresh=0.0, refine_method="NoRefine", capacity=1)
        assert e.value.code == capi.ERR_CAPACITY and e.value.needed == len(full["votes"])


def test_estimate_python_class(capi, scene):
    import misc3d_amd as m3d

    c = scene
    v = m3d.pose_estimation.PPFVoting(c["points"], c["normals"], c["diameter"], c["r_min"])
    res = v.estimate(c["scene_points"], c["scene_normals"], c["reference"], score_thresh=0.0, num_result=2, object_id=5)      # (the default method)
    assert 1 <= len(res) <= 2 and res[0].object_id == 5 and res[0].pose.shape == (4, 4) and res[0].num_votes > 0
    assert _pose_err(res[0].pose, c["T"]) < 1e-9 and 0.0 < res[0].score <= 1.0
    assert np.array_equal(res[0].t, res[0].pose[:3, 3]) and abs(np.linalg.norm(res[0].q) - 1) < 1e-12


def test_refusals_on_the_device_path(capi, scene):
    for kw in (dict(dist_threshold=0.0), dict(angle_threshold=4.0), dict(ratio=-1.0), dict(score_thresh=np.nan),
               dict(rel_dist_sparse_thresh=np.inf), dict(refine_method=5)):
        with pytest.raises(capi.M3DError) as e:
            _estimate(capi, scene, **kw)
        assert e.value.code == capi.ERR_INVALID_ARG, kw
    poses, votes = cu.family("threshold")
    bad = poses.copy()
    bad[0, 0, 3] = np.inf
    with pytest.raises(capi.M3DError) as e:
        capi.ppf_cluster_poses(bad, votes, dist_threshold=cu.R_DIST)
    assert e.value.code == capi.ERR_INVALID_ARG
