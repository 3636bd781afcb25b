"""PPF voting in EdgePoints mode on the GPU: the edge table, the vote and m3d_ppf_estimate_edges of the library against the
contract's restatement (tests/cpp/ppf_ref.c with edge points), integer for integer; the poses against the numpy-longdouble judge.
tests/test_ppf_edge.py holds the restatement to the judge on every input used here, with no pair near a bin edge."""
import ctypes as C
import threading

import numpy as np
import pytest

import ppf_edge_ref_util as eu
import ppf_ref_util as pu

pytestmark = pytest.mark.gpu

INTS = pu.INTS


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pu.PpfRef(tmp_path_factory.mktemp("ppf_edge_ref"))


_ref_model, _ref_vote = pu.ref_model, pu.ref_vote
_model, _vote_on, _vote, _assert_table, _assert_vote = pu.lib_model, pu.lib_vote, pu.forced_vote, pu.assert_table, pu.assert_vote


@pytest.fixture(scope="module")
def expected(ref):
    """the restatement's table and vote of a case, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            c = eu.case(name)
            m = _ref_model(ref, c)
            cache[name] = (m.table(), _ref_vote(m, c))
        return cache[name]
    return get


# ---- the table
@pytest.mark.parametrize("shape", eu.TABLE_SHAPES + (eu.TABLE_LARGE, "coincident"), ids=str)
def test_table_shapes(capi, ref, shape):
    """n != n_e both ways (the index split of a pair), n == n_e (the diagonal that is kept), and coincident points (skipped)"""
    c = eu.coincident_case() if shape == "coincident" else eu.table_case(*shape)
    want = _ref_model(ref, c)
    m = _model(capi, c)
    assert (m.n, m.n_edge) == (len(c["points"]), len(c["edge_points"]))
    t = m.table()
    assert (t["table_size"], t["n_entries"], t["n_neighbors"]) == (want.table_size, want.n_entries, want.n_neighbors)
    assert (t["angle_num"], t["alpha_model_num"], t["dist_num"]) == (16, 31, 21)
    _assert_table(t, want.table())
    if shape == "coincident":
        assert t["n_entries"] == 64 * 64 - 32
    elif shape != eu.TABLE_LARGE:
        assert t["n_entries"] == shape[0] * shape[1]          # (a diameter's worth of distance bins: no pair beyond the table)


# ---- the vote
@pytest.mark.parametrize("device_memory", (False, True), ids=("by_size", "device_memory"))
@pytest.mark.parametrize("name", eu.VOTE_CASES)
def test_vote_cases(capi, expected, name, device_memory):
    """every family with n_e = 320 .. 324, 33 and 61 alpha bins, the full spread, 63 .. 257 scene edge neighbours on every family
    with the gate at 64 / 65, scene edge points on the reference points, and both sides of the LDS limit -- each through the path
    its size chooses and through device memory"""
    c = eu.case(name)
    table, want = expected(name)
    m, (got, stats) = _vote(capi, c, device_memory)
    _assert_table(m.table(), table)
    _assert_vote(c, got, stats, want)
    lds = name != "lds_edge_plus_1" and not device_memory
    assert stats["path"] == (capi.PPF_PATH_LDS if lds else capi.PPF_PATH_DEVICE)
    assert m.info()["path"] == (capi.PPF_PATH_DEVICE if name == "lds_edge_plus_1" else capi.PPF_PATH_LDS)
    assert stats["launches"] == 1 and stats["groups"] == min(len(c["reference"]), 256)
    if name.startswith("count_"):
        count = int(name.rsplit("_", 1)[1])
        assert stats["neighbours_visited"] == count
        assert (stats["increments"] > 0) == (count > 64)      # size_t(0.2 n_e) = 64: 64 neighbours give no vote, 65 the first
    if name == "step_11.25":
        assert m.info()["alpha_model_num"] == 33
    if name in ("step_6", "full_spread_6", "lds_edge"):
        assert m.info()["alpha_model_num"] == 61


@pytest.mark.parametrize("device_memory", (False, True), ids=("lds", "device_memory"))
@pytest.mark.parametrize("max_groups", (1, 3, 5))
def test_workgroups_take_reference_points_in_turn(capi, expected, max_groups, device_memory):
    c = eu.case("family_plate")
    m, (got, stats) = _vote(capi, c, device_memory, max_groups)
    assert stats["groups"] == max_groups
    _assert_vote(c, got, stats, expected("family_plate")[1])


def test_edge_cloud_order_is_free(capi, expected):
    c = dict(eu.case("family_grid"))
    perm = np.random.default_rng(9).permutation(len(c["scene_edge_points"]))
    c["scene_edge_points"], c["scene_edge_normals"] = c["scene_edge_points"][perm], c["scene_edge_normals"][perm]
    for device_memory in (False, True):
        _, (got, stats) = _vote(capi, c, device_memory)
        _assert_vote(c, got, stats, expected("family_grid")[1])


def test_run_to_run_and_capacity(capi, expected):
    c = eu.case("family_sphere")
    want = expected("family_sphere")[1]
    m = _model(capi, c)
    a, b = _vote_on(m, c), _vote_on(m, c)
    for k in INTS + ("poses",):
        assert np.array_equal(a[k], b[k]) and a[k].tobytes() == b[k].tobytes(), k
    K = len(want["votes"])
    assert K > 2
    assert len(_vote_on(m, c, capacity=K)["votes"]) == K
    arrays = [np.ascontiguousarray(c[k]) for k in ("scene_points", "scene_normals", "scene_edge_points", "scene_edge_normals")]
    sp, sn, ep, en = arrays
    refs = np.ascontiguousarray(c["reference"], dtype=np.uint64)
    out = [np.full(K, 0xDEADBEEF, np.uint32) for _ in range(4)]
    poses = np.full((K, 4, 4), 7.0)
    k = C.c_size_t(0)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = capi.lib().m3d_ppf_vote_edges(m.h, p(sp), p(sn), len(sp), p(refs), len(refs), p(ep), p(en), len(ep), K - 1,
                                       C.cast(C.byref(k), C.c_void_p), *(p(o) for o in out), p(poses), None)
    assert rc == capi.ERR_CAPACITY and k.value == K and "maxima" in capi.last_error()
    assert all((o == 0xDEADBEEF).all() for o in out) and (poses == 7.0).all()
    with pytest.raises(capi.M3DError) as e:
        _vote_on(m, c, capacity=0)
    assert e.value.code == capi.ERR_CAPACITY and e.value.needed == K


def test_two_threads_vote_on_one_model(capi, expected):
    c = eu.case("family_random")
    want = expected("family_random")[1]
    m = _model(capi, c)
    results, errors = [None, None], []

    def work(slot):
        try:
            for _ in range(3):
                results[slot] = _vote_on(m, c, stats=True)
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for got, stats in results:
        _assert_vote(c, got, stats, want)


@pytest.mark.parametrize("name", ("family_box", "count_grid_65", "count_random_64", "step_6", "lds_edge_plus_1"))
def test_sampled_mode_is_edge_mode_on_the_sample_itself(capi, ref, name):
    """A SampledPoints case of tests/test_gpu_ppf.py with the sample as the model's edge set and the scene as its own edge cloud
    (the pairs i == j have d2 == 0 and are skipped by rule in either mode): the edge calls give the sampled restatement's table
    and vote, and the library's own sampled result to the byte -- at the gate (65 / 64 neighbours), at 61 alpha bins and through
    device memory (1 176 points).  tests/test_ppf_edge.py shows the same of the restatement and the judge."""
    c = pu.case(name)
    e = pu.with_own_edges(c)
    want = pu.ref_model(ref, c)
    want_vote = pu.ref_vote(want, c)
    m, (got, stats) = _vote(capi, e)
    assert (m.n, m.n_edge) == (len(c["points"]), len(c["points"]))
    t = m.table()
    assert (t["table_size"], t["n_entries"], t["n_neighbors"]) == (want.table_size, want.n_entries, want.n_neighbors)
    _assert_table(t, want.table())
    _assert_vote(e, got, stats, want_vote)
    assert stats["path"] == (capi.PPF_PATH_DEVICE if name == "lds_edge_plus_1" else capi.PPF_PATH_LDS) and stats["launches"] == 1
    sampled, (got_s, stats_s) = _vote(capi, c)
    assert sampled.n_edge == 0
    ts = sampled.table()
    for k in pu.TABLE + ("tmg", "centroid"):
        assert t[k].tobytes() == ts[k].tobytes(), k
    for k in INTS + ("poses",):
        assert got[k].shape == got_s[k].shape and got[k].tobytes() == got_s[k].tobytes(), k
    assert (stats["neighbours_visited"], stats["increments"]) == (stats_s["neighbours_visited"], stats_s["increments"])


def test_mode_mismatches_and_refusals(capi):
    c = eu.case("family_box")
    edge = _model(capi, c)
    sampled = capi.PpfModel(c["points"], c["normals"], c["diameter"], c["r_min"])
    assert (edge.n_edge, sampled.n_edge) == (len(c["edge_points"]), 0)
    with pytest.raises(capi.M3DError) as e:
        edge.vote(c["scene_points"], c["scene_normals"], c["reference"])
    assert e.value.code == capi.ERR_INVALID_ARG and "EdgePoints" in str(e.value)
    with pytest.raises(capi.M3DError) as e:
        _vote_on(sampled, c)
    assert e.value.code == capi.ERR_INVALID_ARG and "SampledPoints" in str(e.value)
    with pytest.raises(capi.M3DError) as e:
        capi.ppf_estimate(edge, c["scene_points"], c["scene_normals"], c["reference"])
    assert e.value.code == capi.ERR_INVALID_ARG and "EdgePoints" in str(e.value)
    with pytest.raises(capi.M3DError) as e:
        capi.ppf_estimate(sampled, c["scene_points"], c["scene_normals"], c["reference"], edge_points=c["scene_edge_points"],
                          edge_normals=c["scene_edge_normals"])
    assert e.value.code == capi.ERR_INVALID_ARG and "SampledPoints" in str(e.value)
    bad = c["scene_edge_normals"].copy()
    bad[3, 1] = np.nan
    with pytest.raises(capi.M3DError) as e:
        edge.vote(c["scene_points"], c["scene_normals"], c["reference"], edge_points=c["scene_edge_points"], edge_normals=bad)
    assert e.value.code == capi.ERR_INVALID_ARG
    with pytest.raises(capi.M3DError) as e:
        edge.vote(c["scene_points"], c["scene_normals"], c["reference"], edge_points=np.zeros((0, 3)), edge_normals=np.zeros((0, 3)))
    assert e.value.code == capi.ERR_INVALID_ARG


def test_sampled_mode_after_an_edge_model_is_unchanged(capi, tmp_path_factory):
    """a SampledPoints model built and voted after an edge model on the same lane: ppf_ref.c's table and vote, integer for integer"""
    e = eu.case("family_box")
    _vote(capi, e)
    ref = pu.PpfRef(tmp_path_factory.mktemp("ppf_ref"))
    for name in ("family_box", "count_plate_65"):
        c = pu.case(name)
        want = ref.model(c["points"], c["normals"], c["diameter"], c["r_min"], c["params"])
        p = c["params"]
        m = capi.PpfModel(c["points"], c["normals"], c["diameter"], c["r_min"], rel_sample_dist=p["rel_sample_dist"],
                          angle_step=p["angle_step"], min_dist_thresh=p["min_dist_thresh"], min_angle_thresh=p["min_angle_thresh"],
                          faster_mode=p["faster_mode"])
        _assert_table(m.table(), want.table())
        got, stats = m.vote(c["scene_points"], c["scene_normals"], c["reference"], stats=True)
        _assert_vote(c, got, stats, want.vote(c["scene_points"], c["scene_normals"], c["reference"]))
        assert m.n_edge == 0


def test_python_class(capi, expected):
    import misc3d_amd as m3d
    c = eu.case("family_box")
    table, want = expected("family_box")
    v = m3d.pose_estimation.PPFVoting(c["points"], c["normals"], c["diameter"], c["r_min"], edge_points=c["edge_points"],
                                      edge_normals=c["edge_normals"])
    assert v.voting_mode == "EdgePoints" and len(v) == len(c["points"]) and np.array_equal(v.centroid, table["centroid"])
    assert np.array_equal(v.table()["entry_i"], table["entry_i"])
    poses, num_votes, corr_mi, reference = v.vote(c["scene_points"], c["scene_normals"], c["reference"],
                                                  edge_points=c["scene_edge_points"], edge_normals=c["scene_edge_normals"])
    assert poses.shape == (len(want["votes"]), 4, 4)
    assert np.array_equal(num_votes, want["votes"]) and np.array_equal(corr_mi, want["model_index"])
    assert np.array_equal(reference, want["ref_pos"])
    with pytest.raises(RuntimeError):
        v.vote(c["scene_points"], c["scene_normals"], c["reference"])                 # an edge model needs the scene's edges
    s = m3d.pose_estimation.PPFVoting(c["points"], c["normals"], c["diameter"], c["r_min"])
    assert s.voting_mode == "SampledPoints"
    with pytest.raises(RuntimeError):
        s.vote(c["scene_points"], c["scene_normals"], c["reference"], edge_points=c["scene_edge_points"],
               edge_normals=c["scene_edge_normals"])


# ---- m3d_ppf_estimate_edges end to end: a flat plate with holes, posed into clutter
# tests/test_ppf_edge.py::test_estimate_case_restated establishes on the CPU that the restatement's top pose on this scene is the
# true pose with either ICP (ESTIMATE_TRUTH there): here the library is held to the restatement and to the truth.
@pytest.fixture(scope="module")
def scene(capi):
    c = eu.estimate_case()
    model = _model(capi, c)
    raw = _vote_on(model, c)
    return dict(c, model=model, raw=raw, centred=np.ascontiguousarray(c["points"] - model.centroid), dist_step=c["diameter"] * 0.05,
                dist_threshold=0.05 * c["diameter"])


@pytest.fixture(scope="module")
def cluster_ref(tmp_path_factory):
    import ppf_cluster_ref_util as cu
    return cu.PcRef(tmp_path_factory.mktemp("ppf_cluster_ref"))


@pytest.fixture(scope="module")
def icp(tmp_path_factory):
    import icp_ref_util as iu
    return iu.IcpRef(tmp_path_factory.mktemp("icp_ref"))


def _pose_err(A, B):
    return float(np.abs(np.asarray(A) - np.asarray(B)).max()) if len(A) else 0.0


def test_raw_vote_of_the_estimate_scene(ref, scene):
    want = _ref_vote(_ref_model(ref, scene), scene)
    for k in INTS:
        assert np.array_equal(scene["raw"][k], want[k]), k
    assert len(want["votes"]) > 0


@pytest.mark.parametrize("method", ("PointToPlane", "PointToPoint", "NoRefine"))
def test_estimate_against_the_restatement(capi, ref, cluster_ref, icp, scene, method):
    """K1 - K7 composed from the clustering and ICP restatements on the raw poses (the ICP against the scene SAMPLE), K8's scores
    from ppf_ref.c: expected = ratio n n"""
    import ppf_cluster_ref_util as cu
    s = scene
    n = len(s["points"])
    got = capi.ppf_estimate(s["model"], s["scene_points"], s["scene_normals"], s["reference"], edge_points=s["scene_edge_points"],
                            edge_normals=s["scene_edge_normals"], angle_threshold=cu.ANGLE, score_thresh=0.0, refine_method=method)
    want = cu.estimate_ref(cluster_ref, icp, s["raw"]["poses"], s["raw"]["votes"], s["centred"], s["model"].centroid, s["scene_points"],
                           s["scene_normals"], s["dist_step"], s["dist_threshold"], score_thresh=0.0, refine_method=method)
    scores, keep = ref.scores(want["votes"], 0.6, n, 0.0, 10)
    print("%s: %d results, votes %s, scores %s" % (method, len(got["votes"]), list(got["votes"]), list(got["scores"])))
    # one vote, and the same one: the estimate runs the vote on the lane it holds, once
    assert got["stats"]["n_raw"] == len(scene["raw"]["votes"])
    assert got["stats"]["vote"]["launches"] == 1
    print("pose differences to the restatement:", [_pose_err(a, b) for a, b in zip(got["poses"], want["poses"])])
    print("top pose to the truth:", _pose_err(got["poses"][0], s["T"]) if len(got["poses"]) else None)
    assert len(got["votes"]) == keep == len(want["votes"]) >= 1
    assert np.array_equal(got["votes"], want["votes"])
    assert np.array_equal(got["scores"], scores[:keep])           # equal as doubles
    assert np.array_equal(got["scores"], np.minimum(1.0, got["votes"].astype(np.float64) / ((0.6 * n) * n)))
    assert _pose_err(got["poses"], want["poses"]) < 1e-9
    assert _pose_err(got["t"], want["t"]) < 1e-9 and _pose_err(got["q"], want["q"]) < 1e-9
    assert got["stats"]["icp_calls"] == (0 if method == "NoRefine" else len(want["refined"]))
    if method != "NoRefine":
        assert _pose_err(got["poses"][0], s["T"]) < 1e-9          # the top pose is the true pose
    # E9 against K8: a threshold of twice the score cuts the result; the SampledPoints score (x 4) would have passed it
    none = capi.ppf_estimate(s["model"], s["scene_points"], s["scene_normals"], s["reference"], edge_points=s["scene_edge_points"],
                             edge_normals=s["scene_edge_normals"], angle_threshold=cu.ANGLE, score_thresh=2.0 * float(scores[0]),
                             refine_method="NoRefine")
    assert 4.0 * scores[0] < 1.0 and len(none["votes"]) == 0
    # the cut by score: a threshold between the first two distinct scores keeps the results above it
    if keep > 1 and scores[0] > scores[keep - 1]:
        thr = 0.5 * (scores[0] + scores[keep - 1])
        cut = capi.ppf_estimate(s["model"], s["scene_points"], s["scene_normals"], s["reference"], edge_points=s["scene_edge_points"],
                                edge_normals=s["scene_edge_normals"], angle_threshold=cu.ANGLE, score_thresh=thr, refine_method="NoRefine")
        assert len(cut["votes"]) == ref.scores(want["votes"], 0.6, n, thr, 10)[1]


def test_two_threads_estimate_on_one_model(capi, scene):
    """two threads, three estimates each (default refinement) on one model: every result is the single-threaded call's"""
    kw = dict(edge_points=scene["scene_edge_points"], edge_normals=scene["scene_edge_normals"], score_thresh=0.0)
    args = (scene["model"], scene["scene_points"], scene["scene_normals"], scene["reference"])
    want = capi.ppf_estimate(*args, **kw)
    assert len(want["votes"]) >= 1 and want["stats"]["icp_calls"] >= 1
    results, errors = [[], []], []

    def work(slot):
        try:
            for _ in range(3):
                results[slot].append(capi.ppf_estimate(*args, **kw))
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


def test_estimate_python_class(capi, scene):
    import misc3d_amd as m3d
    c = scene
    v = m3d.pose_estimation.PPFVoting(c["points"], c["normals"], c["diameter"], c["r_min"], edge_points=c["edge_points"],
                                      edge_normals=c["edge_normals"])
    res = v.estimate(c["scene_points"], c["scene_normals"], c["reference"], edge_points=c["scene_edge_points"],
                     edge_normals=c["scene_edge_normals"], score_thresh=0.0, num_result=2, object_id=5)
    assert 1 <= len(res) <= 2 and res[0].object_id == 5 and res[0].pose.shape == (4, 4) and res[0].num_votes > 0
    assert _pose_err(res[0].pose, c["T"]) < 1e-9 and 0.0 < res[0].score <= 1.0 and abs(np.linalg.norm(res[0].q) - 1) < 1e-12
