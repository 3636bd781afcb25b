"""PPF voting on the GPU: the table and the vote of the library against the contract's restatement (tests/cpp/ppf_ref.c), integer
for integer; the poses against the numpy-longdouble judge.  tests/test_ppf.py holds the restatement to the judge on every input
used here, with no pair near a bin edge."""
import ctypes as C
import threading

import numpy as np
import pytest

import ppf_ref_util as pu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pu.PpfRef(tmp_path_factory.mktemp("ppf_ref"))


@pytest.fixture(scope="module")
def expected(ref):
    """the restatement's table and vote of a case, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            c = pu.case(name)
            m = pu.ref_model(ref, c)
            cache[name] = (m.table(), pu.ref_vote(m, c))
        return cache[name]
    return get


_model, _vote, _assert_table, _assert_vote = pu.lib_model, pu.forced_vote, pu.assert_table, pu.assert_vote


@pytest.mark.parametrize("n", pu.TABLE_SIZES + (pu.TABLE_LARGE,))
def test_table_sizes(capi, ref, n):
    pts, nrm, diameter, r_min = pu.model_case("random", n, pu.TABLE_LARGE_SEED if n == pu.TABLE_LARGE else None)
    want = ref.model(pts, nrm, diameter, r_min, pu.params())
    m = capi.PpfModel(pts, nrm, diameter, r_min)
    t = m.table()
    assert (t["table_size"], t["n_entries"], t["n_neighbors"]) == (want.table_size, want.n_entries, want.n_neighbors)
    assert (t["angle_num"], t["alpha_model_num"], t["dist_num"]) == (16, 31, 21)
    _assert_table(t, want.table())


@pytest.mark.parametrize("device_memory", (False, True), ids=("by_size", "device_memory"))
@pytest.mark.parametrize("name", pu.VOTE_CASES)
def test_vote_cases(capi, expected, name, device_memory):
    """every family, 33 and 61 alpha bins, the full spread, 63 .. 257 neighbours on every family with the gate at 64 / 65, one
    reference point, the undefined places and both sides of the LDS limit -- each through the path its size chooses and through
    device memory"""
    c = pu.case(name)
    table, want = expected(name)
    m, (got, stats) = _vote(capi, c, device_memory)
    _assert_table(m.table(), table)
    _assert_vote(c, got, stats, want)
    lds = name != "lds_edge_plus_1" and not device_memory
    assert stats["path"] == (capi.PPF_PATH_LDS if lds else capi.PPF_PATH_DEVICE)
    assert m.info()["path"] == (capi.PPF_PATH_DEVICE if name == "lds_edge_plus_1" else capi.PPF_PATH_LDS)
    assert stats["launches"] == 1 and stats["groups"] == min(len(c["reference"]), 256)
    if name.startswith("count_"):
        assert (stats["increments"] > 0) == (int(name.rsplit("_", 1)[1]) > 64)
    if name == "step_11.25":
        assert m.info()["alpha_model_num"] == 33
    if name in ("step_6", "full_spread_6", "lds_edge"):
        assert m.info()["alpha_model_num"] == 61


def test_65_alpha_bins_are_refused(capi):
    c = pu.case("family_box")
    with pytest.raises(capi.M3DError) as e:
        capi.PpfModel(c["points"], c["normals"], c["diameter"], c["r_min"], angle_step=5.625 * pu.DEG)
    assert e.value.code == capi.ERR_INVALID_ARG


@pytest.mark.parametrize("device_memory", (False, True), ids=("lds", "device_memory"))
@pytest.mark.parametrize("max_groups", (1, 3, 5))
def test_workgroups_take_reference_points_in_turn(capi, expected, max_groups, device_memory):
    """12 reference points over 1, 3 and 5 workgroups: each clears its flags and accumulators between its points"""
    c = pu.case("family_plate")
    m, (got, stats) = _vote(capi, c, device_memory, max_groups)
    assert stats["groups"] == max_groups
    _assert_vote(c, got, stats, expected("family_plate")[1])


def test_scene_order_is_free(capi, expected):
    c = dict(pu.case("family_grid"))
    rng = np.random.default_rng(9)
    perm = rng.permutation(len(c["scene_points"]))
    where = np.empty(len(perm), np.int64)
    where[perm] = np.arange(len(perm))
    c["scene_points"], c["scene_normals"] = c["scene_points"][perm], c["scene_normals"][perm]
    c["reference"] = where[c["reference"]]
    for device_memory in (False, True):
        _, (got, stats) = _vote(capi, c, device_memory)
        _assert_vote(c, got, stats, expected("family_grid")[1])


def test_run_to_run_and_capacity(capi, expected):
    c = pu.case("family_sphere")
    want = expected("family_sphere")[1]
    m = _model(capi, c)
    a = m.vote(c["scene_points"], c["scene_normals"], c["reference"])
    b = m.vote(c["scene_points"], c["scene_normals"], c["reference"])
    for k in pu.INTS + ("poses",):
        assert np.array_equal(a[k], b[k]) and a[k].tobytes() == b[k].tobytes(), k
    K = len(want["votes"])
    assert K > 2
    # exactly enough room, and one entry short: a status of its own, the needed count, nothing written
    assert len(m.vote(c["scene_points"], c["scene_normals"], c["reference"], capacity=K)["votes"]) == K
    sp, sn = np.ascontiguousarray(c["scene_points"]), np.ascontiguousarray(c["scene_normals"])
    refs = np.ascontiguousarray(c["reference"], dtype=np.uint64)
    out = [np.full(K, 0xDEADBEEF, np.uint32) for _ in range(4)]
    poses = np.full((K, 4, 4), 7.0)
    k = C.c_size_t(0)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = capi.lib().m3d_ppf_vote(m.h, p(sp), p(sn), len(sp), p(refs), len(refs), K - 1, C.cast(C.byref(k), C.c_void_p),
                                 *(p(o) for o in out), p(poses), None)
    assert rc == capi.ERR_CAPACITY and k.value == K and "maxima" in capi.last_error()
    assert all((o == 0xDEADBEEF).all() for o in out) and (poses == 7.0).all()
    with pytest.raises(capi.M3DError) as e:
        m.vote(c["scene_points"], c["scene_normals"], c["reference"], capacity=0)
    assert e.value.code == capi.ERR_CAPACITY and e.value.needed == K


def test_more_maxima_than_the_first_launch_has_room_for(capi):
    """The first launch has room for max(4096, 4 n_ref) maxima; beyond it the vote counts them and launches once more.  The
    1 200-point box of the estimate scene with every point of its copy a reference point has 7 177 maxima (counted with the
    restatement), more than 4 800: two launches.  A maximum belongs to its reference position alone, so the same vote taken in
    three parts of 400 reference points (under 2 500 maxima and one launch each) is the whole, part after part."""
    import ppf_cluster_ref_util as cu
    c = cu.estimate_case()
    _, _, where = pu.scene_of(c["points"], c["normals"], c["T"], 1500, 3)
    refs = np.sort(where)
    m = capi.PpfModel(c["points"], c["normals"], c["diameter"], c["r_min"])
    whole, stats = m.vote(c["scene_points"], c["scene_normals"], refs, stats=True)
    assert stats["launches"] == 2 and len(whole["votes"]) == 7177 > max(4096, 4 * len(refs))
    parts = [m.vote(c["scene_points"], c["scene_normals"], refs[lo:lo + 400], stats=True) for lo in (0, 400, 800)]
    assert [st["launches"] for _, st in parts] == [1, 1, 1] and all(len(r["votes"]) <= 4096 for r, _ in parts)
    assert sum(st["neighbours_visited"] for _, st in parts) == stats["neighbours_visited"]
    assert sum(st["increments"] for _, st in parts) == stats["increments"]
    assert np.array_equal(np.concatenate([r["ref_pos"] + 400 * k for k, (r, _) in enumerate(parts)]), whole["ref_pos"])
    for k in ("model_index", "alpha_index", "votes", "poses"):
        joined = np.concatenate([r[k] for r, _ in parts])
        assert joined.shape == whole[k].shape and joined.tobytes() == whole[k].tobytes(), k


def test_two_threads_vote_on_one_model(capi, expected):
    c = pu.case("family_random")
    want = expected("family_random")[1]
    m = _model(capi, c)
    results, errors = [None, None], []

    def work(slot):
        try:
            for _ in range(3):
                results[slot] = m.vote(c["scene_points"], c["scene_normals"], c["reference"], stats=True)
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


def test_python_class(capi, expected):
    import misc3d_amd as m3d
    c = pu.case("family_box")
    table, want = expected("family_box")
    v = m3d.pose_estimation.PPFVoting(c["points"], c["normals"], c["diameter"], c["r_min"])
    assert len(v) == len(c["points"]) and np.array_equal(v.centroid, table["centroid"])
    assert np.array_equal(v.table()["entry_i"], table["entry_i"])
    poses, num_votes, corr_mi, reference = v.vote(c["scene_points"], c["scene_normals"], c["reference"])
    assert poses.shape == (len(want["votes"]), 4, 4)
    assert np.array_equal(num_votes, want["votes"]) and np.array_equal(corr_mi, want["model_index"])
    assert np.array_equal(reference, want["ref_pos"])
    with pytest.raises(RuntimeError):
        m3d.pose_estimation.PPFVoting(c["points"], c["normals"], c["diameter"], c["r_min"], angle_step=5.625 * pu.DEG)


def test_end_to_end_vote_then_l1_icp(capi):
    """a model posed into clutter: raw poses, then the best-voted one through point-to-plane ICP with L1 weights ends within
    1e-3 of the true pose, once shifted by the centroid"""
    import misc3d_amd as m3d
    pts, nrm, diameter, r_min, sp, sn, ref, T = pu.vote_case("box", n=1200, n_ref=24, clutter=800)
    v = m3d.pose_estimation.PPFVoting(pts, nrm, diameter, r_min)
    poses, num_votes, _, _ = v.vote(sp, sn, ref)
    assert len(num_votes) > 0
    best = poses[int(np.argmax(num_votes))]                  # (the first of the best-voted)
    print("raw pose off by", np.abs(best @ _shift(-v.centroid) - T).max())
    refined, info = m3d.registration_icp(pts - v.centroid, (sp, sn), 0.1 * diameter, best, max_iteration=100,
                                         relative_fitness=1e-9, relative_rmse=1e-9, estimation="point_to_plane_l1")
    err = np.abs(refined @ _shift(-v.centroid) - T).max()
    print("refined pose off by", err, info)
    assert err < 1e-3


def _shift(t):
    S = np.eye(4)
    S[:3, 3] = t
    return S
