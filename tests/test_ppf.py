"""PPF voting without a GPU: the contract's restatement (tests/cpp/ppf_ref.c) on hand cases and against the independent
numpy-longdouble judge on every input the GPU tests use, the host build of the kernels' arithmetic (m3d_ppf_fp.hpp), argument
validation and the Python class."""
import os
import subprocess

import numpy as np
import pytest

import ppf_ref_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEG = np.pi / 180.0


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pu.PpfRef(tmp_path_factory.mktemp("ppf_ref"))


@pytest.fixture(scope="module")
def tables(ref):
    """sizes and edge tables alone (no points): 12 degrees, faster mode and not"""
    z = np.zeros((0, 3))
    return ref.model(z, z, 1.0, 0.3, pu.params()), ref.model(z, z, 1.0, 0.3, pu.params(faster_mode=False))


def test_mirror_header_on_the_host(tmp_path):
    """m3d_ppf_fp.hpp compiled by g++ without contraction: hand-computed bins, edge values included"""
    exe = str(tmp_path / "test_ppf_mirror")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "test_ppf_mirror.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


def test_cpp_mirror_header_compiles(tmp_path):
    src = tmp_path / "use_ppf_voting.cpp"
    src.write_text("#include <misc3d/pose_estimation/ppf_voting.h>\n"
                   "size_t f(const misc3d::pose_estimation::PPFVoting& v) { return v.Size(); }\n")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_sizes(tables):
    m, _ = tables
    assert (m.angle_num, m.alpha_num, m.dist_num, m.table_size) == (16, 31, 21, 16 ** 3 * 21)
    for step, bins in ((11.25, 33), (6.0, 61), (5.625, 65)):
        assert pu.sizes(1.0, pu.params(angle_step=step * DEG))["alpha_num"] == bins


def test_frame_by_hand(ref):
    # a normal along +x: no rotation; the frame moves the point to the origin
    T = ref.frame([0.2, -0.1, 0.4], [1.0, 0.0, 0.0])
    assert np.array_equal(T, np.array([[1, 0, 0, -0.2], [0, 1, 0, 0.1], [0, 0, 1, -0.4], [0, 0, 0, 1.0]]))
    # a normal along +z: a quarter turn about +y takes it to +x
    T = ref.frame([0.0, 0.0, 2.0], [0.0, 0.0, 1.0])
    assert np.allclose(T[:3, :3] @ [0, 0, 1.0], [1, 0, 0], atol=1e-15) and np.allclose(T[:3, :3] @ [0, 1.0, 0], [0, 1, 0], atol=1e-15)
    assert np.allclose(T[:3, 3], [-2.0, 0, 0], atol=1e-15)
    # any normal goes to +x, the point to the origin, and the judge's own construction agrees
    rng = np.random.default_rng(3)
    for _ in range(20):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        p = rng.normal(size=3)
        T = ref.frame(p, n)
        assert np.allclose(T[:3, :3] @ n, [1, 0, 0], atol=1e-14) and np.allclose(T[:3, :3] @ p + T[:3, 3], 0, atol=1e-14)
        assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-14)
        assert np.abs(T - pu.judge_frame(p, n).astype(np.float64)).max() < 1e-14


def test_features_by_hand(tables):
    m, _ = tables
    eye = np.eye(4)
    # p0 at the origin with normal +x: acos(0.6) = 53.13 -> 4, acos(0.36) = 68.90 -> 6, acos(0.6) -> 4, 0.5 / 0.05 -> 10, alpha 0 -> 15
    assert m.pair_bins([0, 0, 0], [1, 0, 0], [0.3, 0.4, 0.0], [0.6, 0.0, 0.8], eye) == ((4, 6, 4, 10), 15)
    # the neighbour straight along the normal: f0 = 0; opposite normals: f1 = f2 = 180 degrees -> 15
    assert m.pair_bins([0, 0, 0], [1, 0, 0], [0.2, 0.0, 0.0], [-1, 0, 0], eye)[0] == (0, 15, 15, 4)
    # alpha: the neighbour's (y, z) in the frame: +y -> 0 (bin 15), -z -> +90 degrees (bin 22 or 23: on an edge), +z -> -90
    assert m.pair_bins([0, 0, 0], [1, 0, 0], [0.0, 0.3, 0.01], [0, 0, 1], eye)[1] == 15
    assert m.pair_bins([0, 0, 0], [1, 0, 0], [0.0, 0.1, -0.3], [0, 0, 1], eye)[1] == round((np.arctan2(0.3, 0.1) + np.pi) / (12 * DEG))
    assert m.pair_bins([0, 0, 0], [1, 0, 0], [0.0, -0.3, 0.1], [0, 0, 1], eye)[1] == round((np.arctan2(-0.1, -0.3) + np.pi) / (12 * DEG))
    # the undefined places: d2 == 0 and a distance bin beyond the table are skipped
    assert m.pair_bins([0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0], eye) is None
    assert m.pair_bins([0, 0, 0], [1, 0, 0], [0.9, 0.9, 0.9], [0, 1, 0], eye) is None
    assert m.pair_bins([0, 0, 0], [1, 0, 0], [1.0, 0.0, 0.0], [0, 1, 0], eye)[0][3] == 20


def test_spread_counts(tables):
    fast, full = tables
    assert len(fast.spread([5, 5, 5, 5])) == 24 and len(full.spread([5, 5, 5, 5])) == 81
    assert len(fast.spread([0, 0, 0, 0])) == 2 and len(full.spread([0, 0, 0, 0])) == 16
    assert len(fast.spread([15, 15, 15, 20])) == 16 and len(full.spread([15, 15, 15, 20])) == 16
    assert len(fast.spread([0, 5, 15, 10])) == 12
    sz = pu.sizes(1.0, pu.params())
    for q in ([5, 6, 7, 8], [0, 15, 3, 20], [15, 0, 0, 0]):
        assert list(fast.spread(q)) == pu.spread_cells(q, sz, 2) and list(full.spread(q)) == pu.spread_cells(q, sz, 3)
        assert len(set(full.spread(q))) == len(full.spread(q))
    assert fast.spread([5, 6, 7, 8])[0] == 4 + 16 * (5 + 16 * (6 + 16 * 7))


def _both(ref, acc, thr, nbrs):
    a = ref.local_maximum(acc, thr, nbrs)
    assert a == pu.local_maximum_py(acc, thr, nbrs)
    return a


def test_local_maximum_by_hand(ref):
    alone = [[0], [1], [2]]
    # wrap-around windows: the votes in columns 4 and 0 of a 5-column row meet in the window of column 4 (and of column 0 ...
    acc = np.zeros((3, 5), np.uint32)
    acc[0, 4], acc[0, 0] = 5, 4
    acc[1, 2] = 3
    # ... which comes first: window 0 = a4 + a0 + a1 = 9, window 4 = a3 + a4 + a0 = 9: strict > keeps column 0)
    assert _both(ref, acc, 1, alone) == [(0, 0, 9)]
    acc[0, 3] = 1                      # now window 4 = 10 > window 0 = 9
    assert _both(ref, acc, 1, alone) == [(0, 4, 10)]
    # ties between rows: both are maxima when they are no neighbours; with rows 0 and 1 neighbours the first clears the second
    acc = np.zeros((3, 5), np.uint32)
    acc[0, 1] = acc[1, 3] = 7
    assert _both(ref, acc, 1, alone) == [(0, 0, 7), (1, 2, 7)]       # (a single column's first window is the one to its left)
    assert _both(ref, acc, 1, [[0, 1], [0, 1], [2]]) == [(0, 0, 7)]
    # the global threshold: nothing below it; 0.8 max: rows at or below it are no candidates
    assert _both(ref, acc, 8, alone) == []
    acc[2, 2] = 5                      # 5 <= int(7 * 0.8) = 5
    assert _both(ref, acc, 1, alone) == [(0, 0, 7), (1, 2, 7)]
    acc[2, 2] = 6
    assert _both(ref, acc, 1, alone) == [(0, 0, 7), (1, 2, 7), (2, 1, 6)]
    # suppression by a non-maximum row: row 0 (9) is beaten by its neighbour row 1 (10) yet clears its neighbour row 2 (9),
    # which is no neighbour of row 1 and would otherwise be reported
    acc = np.zeros((3, 5), np.uint32)
    acc[0, 1], acc[1, 1], acc[2, 1] = 9, 10, 9
    assert _both(ref, acc, 1, [[0, 1, 2], [0, 1], [0, 2]]) == [(1, 0, 10)]
    assert _both(ref, acc, 1, [[0, 1], [0, 1], [2]]) == [(1, 0, 10), (2, 0, 9)]


def _assert_ref_equals_judge(ref, c):
    m = ref.model(c["points"], c["normals"], c["diameter"], c["r_min"], c["params"])
    jm = pu.judge_model(c["points"], c["normals"], c["diameter"], c["r_min"], c["params"])
    assert jm["undecided"] == 0          # a condition on the inputs, not a tolerance: no pair near a bin edge
    t = m.table()
    for k in ("cell_offsets", "entry_i", "entry_alpha", "nbr_offsets", "nbr_indices"):
        assert np.array_equal(t[k], jm[k]), k
    assert np.array_equal(t["centroid"], jm["centroid"])
    assert np.abs(t["tmg"] - jm["tmg"].astype(np.float64)).max() < 1e-12
    return m, jm


@pytest.mark.parametrize("n", pu.TABLE_SIZES + (pu.TABLE_LARGE,))
def test_table_restatement_equals_judge(ref, n):
    pts, nrm, diameter, r_min = pu.model_case("random", n, pu.TABLE_LARGE_SEED if n == pu.TABLE_LARGE else None)
    _assert_ref_equals_judge(ref, dict(points=pts, normals=nrm, diameter=diameter, r_min=r_min, params=pu.params()))


@pytest.mark.parametrize("name", pu.VOTE_CASES)
def test_vote_restatement_equals_judge(ref, name):
    c = pu.case(name)
    m, jm = _assert_ref_equals_judge(ref, c)
    v = m.vote(c["scene_points"], c["scene_normals"], c["reference"])
    j = pu.judge_vote(jm, c["r_min"], c["params"], c["scene_points"], c["scene_normals"], c["reference"])
    assert j["undecided"] == 0
    assert list(v["n_searched"]) == j["n_searched"]
    for k in ("ref_pos", "model_index", "alpha_index", "votes"):
        assert list(v[k]) == j[k], k
    if len(j["poses"]):
        assert np.abs(v["poses"] - np.asarray(j["poses"])).max() < 1e-12
    if name.startswith("count_"):
        count, gate = int(name.rsplit("_", 1)[1]), int(0.2 * pu.VOTE_N)
        assert list(v["n_searched"]) == [count] and gate == 64
        assert (v["increments"] > 0) == (count > gate)      # 64 neighbours: no vote; 65: the first vote
    elif name not in ("beyond_dist_num",):
        assert len(v["votes"]) > 0


def test_python_class_exists():
    import misc3d_amd as m3d
    assert m3d.pose_estimation.PPFVoting is m3d.PPFVoting
    for attr in ("centroid", "table", "vote"):
        assert hasattr(m3d.PPFVoting, attr)
    assert "PPFEstimator is not part of this build" in type(m3d.pose_estimation).__doc__


def test_argument_validation_needs_no_gpu(capi):
    pts, nrm, diameter, r_min = pu.model_case("random", 64)

    def refused(*args, **kw):
        with pytest.raises(capi.M3DError) as e:
            capi.PpfModel(*args, **kw)
        return e.value.code

    assert refused(pts[:1], nrm[:1], diameter, r_min) == capi.ERR_INVALID_ARG                    # n < 2
    big = np.zeros((65536, 3))
    assert refused(big, big, diameter, r_min) == capi.ERR_INVALID_ARG                            # n > 65535
    assert refused(pts, nrm, diameter, r_min, angle_step=5.625 * DEG) == capi.ERR_INVALID_ARG    # 65 alpha bins
    assert "alpha_model_num = 65" in capi.last_error()
    bad = pts.copy()
    bad[7, 1] = np.nan
    assert refused(bad, nrm, diameter, r_min) == capi.ERR_INVALID_ARG
    bad = nrm.copy()
    bad[63, 2] = np.inf
    assert refused(pts, bad, diameter, r_min) == capi.ERR_INVALID_ARG
    for d, r in ((0.0, r_min), (diameter, -1.0), (np.nan, r_min)):
        assert refused(pts, nrm, d, r) == capi.ERR_INVALID_ARG
    assert refused(pts, nrm, diameter, r_min, rel_sample_dist=0.0) == capi.ERR_INVALID_ARG
    assert refused(pts, nrm, diameter, r_min, rel_sample_dist=1e-4, angle_step=6 * DEG) == capi.ERR_INVALID_ARG   # table >= 2^24
    with pytest.raises(TypeError):
        capi.ppf_params(no_such_field=1)
    P = capi.ppf_params()
    assert (P.rel_sample_dist, P.min_dist_thresh, P.faster_mode) == (0.05, 1.0 / 3.0, 1)
    assert P.angle_step == 12.0 / 180.0 * np.pi and P.min_angle_thresh == 30.0 / 180.0 * np.pi
    # the vote's checks come before any device work too: a null model
    k = np.zeros(1, np.uint64)
    rc = capi.lib().m3d_ppf_vote(None, None, None, 0, None, 0, 0, k.ctypes.data, None, None, None, None, None, None)
    assert rc == capi.ERR_INVALID_ARG


def test_no_cpu_fallback(capi):
    """valid arguments and no device: an error, never a host computation (with a device: the model is built)"""
    pts, nrm, diameter, r_min = pu.model_case("random", 64)
    if capi.device_count() > 0:
        assert capi.PpfModel(pts, nrm, diameter, r_min).n == 64
        return
    with pytest.raises(capi.M3DError) as e:
        capi.PpfModel(pts, nrm, diameter, r_min)
    assert e.value.code == capi.ERR_DEVICE
