"""PPF voting in EdgePoints mode without a GPU: the contract's restatement (tests/cpp/ppf_ref.c with edge points) on hand cases and
against the independent numpy-longdouble judge on every input the GPU tests use (none of which has a pair near a bin edge), why
rule E1 centres the edge set, SampledPoints as EdgePoints with the sample as its own edge set, the restated estimate of the
end-to-end scene, argument validation and mode refusals through the C ABI, the exported symbols, the C++ mirror and the host steps
of m3d_ppf_prepare_scene."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ppf_edge_ref_util as eu
import ppf_ref_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# What the restatement does on the end-to-end scene (eu.estimate_case: a flat plate with holes in clutter), asserted by
# test_estimate_case_restated -- the truth check of tests/test_gpu_ppf_edge.py is a condition on this input, established here:
# one result; refined by either ICP its pose is the true pose (measured: 4e-16 off), unrefined it is the averaged pose of the
# vote's bins (measured: 0.026 off; half a distance step is 0.03).  The plate's sample has points on the walls of its rim and
# holes: with the face alone every point-to-plane residual is blind to a slide inside the plane, and that ICP ends 0.1 off.
ESTIMATE_TRUTH = {"PointToPlane": 1e-9, "PointToPoint": 1e-9, "NoRefine": 0.03}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pu.PpfRef(tmp_path_factory.mktemp("ppf_edge_ref"))


_ref_model = pu.ref_model


# ---- hand cases: diameter 1, 12 degrees: dist_step 0.05, cell = q0 + 16 (q1 + 16 (q2 + 16 q3))
S0, S1 = [0.0, 0.0, 0.0], [0.0, 0.1, 0.4]                  # two sample points, both with normal +x: their frames only translate
E0, NE0 = [0.3, 0.4, 0.0], [0.6, 0.0, 0.8]                  # one edge point


def _hand(ref, edge_points, edge_normals):
    return ref.model([S0, S1], [[1.0, 0, 0], [1.0, 0, 0]], 1.0, 0.3, pu.params(), edge_points, edge_normals)


def test_two_sample_points_one_edge_point_by_hand(ref):
    """(S0, E0): d = (0.3, 0.4, 0), |d| = 0.5 -> 10; f0 = acos(0.6) = 53.13 -> 4; f1 = acos(0.36) = 68.90 -> 6; f2 = acos(0.6) -> 4;
    alpha = atan2(0, 0.4) = 0 -> bin 15.  (S1, E0): d = (0.3, 0.3, -0.4), |d| = 0.5831 -> 12; f0 = acos(0.5145) = 59.04 -> 5;
    f1 = acos(-0.2401) = 103.89 -> 9; f2 -> 4; alpha = atan2(0.4, 0.3) = 53.13, (53.13 + 180) / 12 = 19.43 -> 19."""
    m = _hand(ref, [E0], [NE0])
    t = m.table()
    cell0 = 4 + 16 * (6 + 16 * (4 + 16 * 10))
    cell1 = 5 + 16 * (9 + 16 * (4 + 16 * 12))
    assert (cell0, cell1) == (42084, 50325) and m.n_entries == 2
    assert list(t["entry_i"]) == [0, 1] and list(t["entry_alpha"]) == [15, 19]
    off = t["cell_offsets"].astype(np.int64)
    assert list(np.nonzero(np.diff(off))[0]) == [cell0, cell1]
    assert np.array_equal(t["centroid"], [0.0, 0.05, 0.2])                  # of the SAMPLE alone
    assert np.array_equal(t["nbr_offsets"], [0, 1, 2])                       # |S1 - S0| = 0.41 > 0.5 r_min: each its own neighbour


def test_an_edge_point_on_a_sample_point_is_skipped(ref):
    """rule U2 under E3: E1 = S1 -- the pair (1, E1) has d2 == 0 and is skipped, (0, E1) is a pair like any other"""
    m = _hand(ref, [E0, S1], [NE0, [0.0, 1.0, 0.0]])
    t = m.table()
    assert m.n_entries == 3 and sorted(t["entry_i"]) == [0, 0, 1]
    # (S0, S1): d = (0, 0.1, 0.4), |d| = 0.4123 -> 8; f0 = acos(0) -> on an edge, not asserted; the entry is there, under i = 0
    assert sum(1 for i in t["entry_i"] if i == 1) == 1


def test_equal_indices_are_pairs(ref):
    """two sample points, two edge points, none coincident: all four pairs, (0, 0) and (1, 1) among them -- the same-set table of
    two points has two"""
    m = _hand(ref, [E0, [0.2, -0.3, 0.1]], [NE0, [0.0, 0.6, 0.8]])
    assert m.n_entries == 4 and list(m.table()["entry_i"]) .count(0) == 2
    same = ref.model([S0, S1], [[1.0, 0, 0], [1.0, 0, 0]], 1.0, 0.3, pu.params())
    assert same.n_entries == 2


# ---- the restatement against the judge on every GPU case
def _assert_ref_equals_judge(ref, c):
    m = _ref_model(ref, c)
    jm = pu.judge_model(c["points"], c["normals"], c["diameter"], c["r_min"], c["params"], c["edge_points"], c["edge_normals"])
    assert jm["undecided"] == 0          # a condition on the inputs, not a tolerance: no pair near a bin edge
    t = m.table()
    for k in pu.TABLE:
        assert np.array_equal(t[k], jm[k]), k
    assert np.array_equal(t["centroid"], jm["centroid"])
    assert np.abs(t["tmg"] - jm["tmg"].astype(np.float64)).max() < 1e-12
    return m, jm


@pytest.mark.parametrize("shape", eu.TABLE_SHAPES + (eu.TABLE_LARGE, "coincident"), ids=str)
def test_table_restatement_equals_judge(ref, shape):
    c = eu.coincident_case() if shape == "coincident" else eu.table_case(*shape)
    m, _ = _assert_ref_equals_judge(ref, c)
    if shape == "coincident":
        assert m.n_entries == 64 * 64 - 32


@pytest.mark.parametrize("name", eu.VOTE_CASES)
def test_vote_restatement_equals_judge(ref, name):
    c = eu.case(name)
    m, jm = _assert_ref_equals_judge(ref, c)
    args = (c["scene_points"], c["scene_normals"], c["reference"], c["scene_edge_points"], c["scene_edge_normals"])
    v = m.vote(*args)
    j = pu.judge_vote(jm, c["r_min"], c["params"], *args)
    assert j["undecided"] == 0
    assert list(v["n_searched"]) == j["n_searched"]
    for k in ("ref_pos", "model_index", "alpha_index", "votes"):
        assert list(v[k]) == j[k], k
    if len(j["poses"]):
        assert np.abs(v["poses"] - np.asarray(j["poses"])).max() < 1e-12
    gate = int(0.2 * len(c["edge_points"]))
    assert gate == 64                                           # n_e = 320 .. 324
    if name.startswith("count_"):
        count = int(name.rsplit("_", 1)[1])
        assert list(v["n_searched"]) == [count]
        assert (v["increments"] > 0) == (count > gate)          # 64 neighbours: no vote; 65: the first vote
    else:
        assert len(v["votes"]) > 0


# ---- why rule E1 centres the edge set
def test_centring_both_sets_recovers_the_pose_and_the_reference_way_does_not(ref):
    """The plate of the end-to-end case moved off the origin and posed by T, no clutter.  With both sets centred (E1) the vote's
    maxima hold a pose of the true one's bin: within 0.1 in every entry once shifted by the centroid (half an angle step is 0.105
    rad, half a distance step 0.03).  With the edge set left uncentred, as ppf_estimation.cpp:588-589 leaves it, the table pairs
    points that are 1.1 apart with edge points around them -- most pairs beyond dist_num -- and the vote finds no such pose."""
    c = eu.estimate_case()
    off = np.array([0.8, -0.5, 0.6])
    pts, ept, T = c["points"] + off, c["edge_points"] + off, c["T"]
    sp, sn = pts @ T[:3, :3].T + T[:3, 3], c["normals"] @ T[:3, :3].T
    ep, en = ept @ T[:3, :3].T + T[:3, 3], c["edge_normals"] @ T[:3, :3].T
    refs = np.arange(0, len(sp), 16)
    errs = {}
    for centre in (True, False):
        m = ref.model(pts, c["normals"], c["diameter"], c["r_min"], c["params"], ept, c["edge_normals"], centre_edges=centre)
        v = m.vote(sp, sn, refs, ep, en)
        S = np.eye(4)
        S[:3, 3] = -m.table()["centroid"]
        errs[centre] = [float(np.abs(P @ S - T).max()) for P in v["poses"]]
    print("errors of the raw poses to the truth: centred min %.3g of %d; uncentred %s" %
          (min(errs[True]), len(errs[True]), "min %.3g of %d" % (min(errs[False]), len(errs[False])) if errs[False] else "no maxima"))
    assert len(errs[True]) > 0 and min(errs[True]) < 0.1
    assert all(e > 0.1 for e in errs[False])


# ---- the two modes are one: SampledPoints is EdgePoints with the sample as its own referred set
@pytest.mark.parametrize("name", pu.OWN_EDGE_CASES)
def test_sampled_mode_is_edge_mode_on_the_sample_itself(ref, name):
    """The pairs i == j have d2 == 0 and are skipped by rule U2 in either mode, so a model trained with its sample as its edge set
    and voted with the scene as its own edge cloud is the sampled model: the table, every integer of the vote, the counters and
    the poses to the byte, in the restatement; the integers in the judge."""
    c = pu.case(name)
    e = pu.with_own_edges(c)
    sampled, edge = pu.ref_model(ref, c), pu.ref_model(ref, e)
    n = len(c["points"])
    assert (sampled.n_e, edge.n_e) == (0, n)
    assert (edge.table_size, edge.n_entries, edge.n_neighbors) == (sampled.table_size, sampled.n_entries, sampled.n_neighbors)
    assert sampled.n_entries == n * (n - 1)                     # (no pair beyond the table in these cases)
    ts, te = sampled.table(), edge.table()
    for k in ts:
        assert te[k].tobytes() == ts[k].tobytes(), k
    vs, ve = pu.ref_vote(sampled, c), pu.ref_vote(edge, e)
    for k in pu.INTS + ("n_searched", "poses"):
        assert ve[k].shape == vs[k].shape and ve[k].tobytes() == vs[k].tobytes(), k
    assert (ve["visited"], ve["increments"]) == (vs["visited"], vs["increments"])
    assert len(vs["votes"]) > 0 or name == "count_random_64"    # 64 neighbours: below the gate, no vote
    js = pu.judge_model(c["points"], c["normals"], c["diameter"], c["r_min"], c["params"])
    je = pu.judge_model(c["points"], c["normals"], c["diameter"], c["r_min"], c["params"], e["edge_points"], e["edge_normals"])
    assert js["undecided"] == je["undecided"] == 0 and (js["n_e"], je["n_e"]) == (0, n)
    for k in pu.TABLE:
        assert np.array_equal(je[k], js[k]) and np.array_equal(je[k], ts[k]), k
    scene = (c["scene_points"], c["scene_normals"], c["reference"])
    vjs = pu.judge_vote(js, c["r_min"], c["params"], *scene)
    vje = pu.judge_vote(je, c["r_min"], c["params"], *scene, e["scene_edge_points"], e["scene_edge_normals"])
    assert vjs["undecided"] == vje["undecided"] == 0
    for k in pu.INTS + ("n_searched",):
        assert vje[k] == vjs[k] == list(vs[k]), k


# ---- the restated estimate of the end-to-end scene (K1 - K7 from the clustering and ICP restatements, K8's scores from E9)
def test_estimate_case_restated(ref, tmp_path_factory):
    import icp_ref_util as iu
    import ppf_cluster_ref_util as cu
    tmp = tmp_path_factory.mktemp("estimate_refs")
    pc, icp = cu.PcRef(tmp), iu.IcpRef(tmp)
    c = eu.estimate_case()
    m = _ref_model(ref, c)
    raw = m.vote(c["scene_points"], c["scene_normals"], c["reference"], c["scene_edge_points"], c["scene_edge_normals"])
    cen = m.table()["centroid"]
    n = len(c["points"])
    for method, bar in ESTIMATE_TRUTH.items():
        want = cu.estimate_ref(pc, icp, raw["poses"], raw["votes"], np.ascontiguousarray(c["points"] - cen), cen, c["scene_points"],
                               c["scene_normals"], c["diameter"] * 0.05, 0.05 * c["diameter"], score_thresh=0.0, refine_method=method)
        err = float(np.abs(want["poses"][0] - c["T"]).max())
        print(method, "votes", list(want["votes"]), "top pose to the truth", err)
        assert len(want["votes"]) >= 1 and err < bar
        scores, keep = ref.scores(want["votes"], 0.6, n, 0.0, 10)
        assert keep == len(want["votes"]) and scores[0] == min(1.0, float(want["votes"][0]) / ((0.6 * n) * n))
        # E9 against K8: the SampledPoints score of the same votes is four times as large (below the cap)
        sampled = pc.finish(want["refined"], want["votes"], cen, 0.6, n, 0.0, 10)["scores"]
        assert sampled[0] == min(1.0, float(want["votes"][0]) / (((0.6 * n) * n) * 0.25)) and scores[0] < sampled[0]
        assert ref.scores(want["votes"], 0.6, n, 2.0 * scores[0], 10)[1] == 0     # the cut


# ---- the C ABI without a device
def test_symbols_exported_and_bound(capi):
    for name in ("m3d_ppf_model_create_edges", "m3d_ppf_model_edge_size", "m3d_ppf_vote_edges", "m3d_ppf_estimate_edges",
                 "m3d_ppf_prepare_scene"):
        f = getattr(capi.lib(), name)
        assert f.argtypes is not None, name
    assert callable(capi.ppf_prepare_scene)
    import misc3d_amd as m3d
    assert callable(m3d.pose_estimation.ppf_prepare_scene) and isinstance(m3d.PPFVoting.voting_mode, property)
    assert "PPFEstimator is not part of this build" in type(m3d.pose_estimation).__doc__
    assert capi.lib().m3d_ppf_model_edge_size(None) == 0


def test_argument_validation_needs_no_gpu(capi):
    pts, nrm, ept, enr, diameter = eu.split_family("random", 64, 48, 3)
    r_min = 0.45 * diameter

    def refused(*args, **kw):
        with pytest.raises(capi.M3DError) as e:
            capi.PpfModel(*args, **kw)
        return e.value.code

    z = np.zeros((0, 3))
    assert refused(pts, nrm, diameter, r_min, edge_points=z, edge_normals=z) == capi.ERR_INVALID_ARG                 # n_e = 0
    assert "edge points" in capi.last_error()
    big = np.zeros((65536, 3))
    assert refused(pts, nrm, diameter, r_min, edge_points=big, edge_normals=big) == capi.ERR_INVALID_ARG             # n_e = 65536
    bad = enr.copy()
    bad[47, 2] = np.inf
    assert refused(pts, nrm, diameter, r_min, edge_points=ept, edge_normals=bad) == capi.ERR_INVALID_ARG             # non-finite
    bad = ept.copy()
    bad[0, 0] = np.nan
    assert refused(pts, nrm, diameter, r_min, edge_points=bad, edge_normals=enr) == capi.ERR_INVALID_ARG
    assert refused(pts[:1], nrm[:1], diameter, r_min, edge_points=ept, edge_normals=enr) == capi.ERR_INVALID_ARG     # n < 2 as M1
    # n n_e > 2^28: finite points, so the size is what refuses -- as the sampled table's cap, M3D_ERR_DEVICE, with no device touched
    rng = np.random.default_rng(1)
    many, edges = rng.uniform(-1, 1, size=(16385, 3)), rng.uniform(-1, 1, size=(16384, 3))
    assert 16385 * 16384 > 2 ** 28
    assert refused(many, many, diameter, r_min, edge_points=edges, edge_normals=edges) == capi.ERR_DEVICE
    assert "2^28" in capi.last_error()
    with pytest.raises(ValueError):
        capi.PpfModel(pts, nrm, diameter, r_min, edge_points=ept)
    # the votes' checks come before any device work too: a null model through either edge call
    k = np.zeros(1, np.uint64)
    rc = capi.lib().m3d_ppf_vote_edges(None, None, None, 0, None, 0, None, None, 0, 0, k.ctypes.data, None, None, None, None, None, None)
    assert rc == capi.ERR_INVALID_ARG
    rc = capi.lib().m3d_ppf_estimate_edges(None, None, None, 0, None, 0, None, None, 0, None, 0, k.ctypes.data, None, None, None, None,
                                           None, None)
    assert rc == capi.ERR_INVALID_ARG
    # m3d_ppf_prepare_scene: no points
    with pytest.raises(capi.M3DError) as e:
        capi.ppf_prepare_scene(z, None, 1.0, 0.05, 0.05)
    assert e.value.code == capi.ERR_INVALID_ARG and "There is no scene point clouds." in str(e.value)
    with pytest.raises(capi.M3DError) as e:
        capi.ppf_prepare_scene(np.full((5, 3), np.nan), None, 1.0, 0.05, 0.05)
    assert e.value.code == capi.ERR_INVALID_ARG and "There is no scene point clouds." in str(e.value)


def test_a_vote_through_the_wrong_call_is_refused(capi):
    """the mode is decided before any device is touched; a model needs a device to exist, so without one the model's creation is
    what fails (tests/test_gpu_ppf_edge.py::test_mode_mismatches_and_refusals runs the same refusals on the GPU)"""
    c = eu.case("family_box")
    kw = dict(edge_points=c["edge_points"], edge_normals=c["edge_normals"])
    if capi.device_count() == 0:
        with pytest.raises(capi.M3DError) as e:
            capi.PpfModel(c["points"], c["normals"], c["diameter"], c["r_min"], **kw)
        assert e.value.code == capi.ERR_DEVICE               # valid arguments and no device: an error, never a host computation
        return
    edge = capi.PpfModel(c["points"], c["normals"], c["diameter"], c["r_min"], **kw)
    with pytest.raises(capi.M3DError) as e:
        edge.vote(c["scene_points"], c["scene_normals"], c["reference"])
    assert e.value.code == capi.ERR_INVALID_ARG and "EdgePoints" in str(e.value)
    sampled = capi.PpfModel(c["points"], c["normals"], c["diameter"], c["r_min"])
    with pytest.raises(capi.M3DError) as e:
        sampled.vote(c["scene_points"], c["scene_normals"], c["reference"], edge_points=c["scene_edge_points"],
                     edge_normals=c["scene_edge_normals"])
    assert e.value.code == capi.ERR_INVALID_ARG and "SampledPoints" in str(e.value)


# ---- the C++ mirror and the host steps of m3d_ppf_prepare_scene
def test_cpp_mirror_header_compiles(tmp_path):
    src = tmp_path / "use_ppf_voting_edges.cpp"
    src.write_text(
        "#include <misc3d/pose_estimation/ppf_voting.h>\n"
        "using namespace misc3d::pose_estimation;\n"
        "size_t f(PPFVoting& v, const double* p, const double* n, size_t k, const std::vector<size_t>& r) {\n"
        "    v.TrainEdges(p, n, k, p, n, k, 1.0, 0.4);\n"
        "    std::vector<VotedPose> a = v.VoteEdges(p, n, k, r, p, n, k);\n"
        "    std::vector<Pose6D> b = v.EstimateEdges(p, n, k, r, p, n, k, v.DefaultClusterParams());\n"
        "    PreparedScene s = PPFVoting::PrepareScene(p, nullptr, k, 1.0, 0.05, 0.05, 0.02, 30);\n"
        "    return a.size() + b.size() + s.edge_indices.size() + v.EdgeSize() + (v.IsEdgeMode() ? 1 : 0);\n"
        "}\n")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_prepare_scene_host_steps(tmp_path):
    """m3d_ppf_prepare.hpp compiled by g++ without contraction: the non-finite rows dropped, NormalConsistent by hand"""
    exe = str(tmp_path / "test_ppf_prepare_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "test_ppf_prepare_host.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
