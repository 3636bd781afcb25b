"""PPF pose clustering without a GPU: the contract's restatement (tests/cpp/ppf_cluster_ref.c) on hand cases of K2, K4 and K8,
against the independent numpy-longdouble judge and against a line-by-line simulation of the reference's GatherPose on every
input family the GPU tests use; the conditions those families must meet (no undecided pair, eigen gaps, a real bridge pose);
the Jacobi solver and MatToQuat of m3d_ppf_cluster_fp.hpp; argument validation."""
import os
import subprocess

import numpy as np
import pytest

import ppf_cluster_ref_util as cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEG = np.pi / 180.0


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return cu.PcRef(tmp_path_factory.mktemp("ppf_cluster_ref"))


@pytest.fixture(scope="module")
def restated(ref):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ref.cluster(*cu.family(name))
        return cache[name]
    return get


def _line(n, spacing, votes):
    """n poses with one rotation on the x axis, `spacing` (in units of the distance threshold) apart"""
    R = cu.rot([0.0, 0.0, 1.0], 0.3)
    return np.asarray([cu._pose(R, [k * spacing * cu.R_DIST, 0.0, 0.0]) for k in range(n)]), np.asarray(votes, dtype=np.uint32)


# ---- hand cases
def test_k2_threshold_by_hand(ref):
    assert [ref.threshold(v) for v in (41, 40, 3, 1, 0)] == [20, 20, 1, 0, 0]      # size_t(votes 0.5)
    poses, votes = _line(6, 10.0, [41, 20, 19, 21, 20, 19])
    r = ref.cluster(poses, votes)
    assert list(r["order"]) == [0, 3, 1, 4]            # votes descending, ties by input index; the two 19s are cut
    assert r["stats"]["n_valid"] == 4 and r["stats"]["clusters_t"] == 0 and r["min_num_pt_t"] == 3


def test_k4_by_hand(ref):
    # five poses 0.6 r apart: the counts are 2 3 3 3 2, min_num_pt = int(max(6, 3) / 2.0) = 3: three cores, two border poses, one
    # cluster; votes descending along the line, so positions are input indices
    poses, votes = _line(5, 0.6, [50, 49, 48, 47, 46])
    r = ref.cluster(poses, votes)
    assert list(r["count_t"]) == [2, 3, 3, 3, 2] and r["min_num_pt_t"] == 3
    assert list(r["label_t"]) == [0] * 5 and list(r["cluster_votes"]) == [240]
    assert list(r["count_r"]) == [2, 3, 3, 3, 2] and list(r["label_r"]) == [0] * 5 and list(r["min_num_pt_r"]) == [3]
    assert list(r["avg_votes"]) == [240] and list(r["avg_cluster"]) == [0]
    assert np.abs(r["avg_poses"][0][:3, 3] - [1.2 * cu.R_DIST, 0, 0]).max() < 1e-15
    # nine poses in one place and one 0.9 r away beside two of its own 0.9 r further: counts 10 x 9, 12, 3, 3; min_num_pt =
    # int(12 / 2.0) = 6; the pose with 12 neighbours is a core, the two beyond it (count 3) are border poses of the one cluster
    R = cu.rot([0.0, 0.0, 1.0], 0.3)
    P = [cu._pose(R, [0, 0, 0])] * 9 + [cu._pose(R, [0.9 * cu.R_DIST, 0, 0])] + [cu._pose(R, [1.8 * cu.R_DIST, 0, 0])] * 2
    r = ref.cluster(np.asarray(P), np.arange(40, 28, -1))
    assert list(r["count_t"]) == [10] * 9 + [12, 3, 3] and r["min_num_pt_t"] == 6
    assert list(r["label_t"]) == [0] * 12
    # a pose with no core neighbour is dropped: the same with the far pair moved out of reach of everything
    P[10] = P[11] = cu._pose(R, [5 * cu.R_DIST, 0, 0])
    r = ref.cluster(np.asarray(P), np.arange(40, 28, -1))
    assert list(r["count_t"]) == [10] * 10 + [2, 2] and r["min_num_pt_t"] == 5 and list(r["label_t"]) == [0] * 10 + [-1, -1]
    assert list(r["label_r"]) == [0] * 10 + [-1, -1] and list(r["count_r"]) == [10] * 10 + [0, 0]


def test_k8_by_hand(ref):
    I = np.eye(4)
    A, B, Cc = I.copy(), I.copy(), I.copy()
    A[:3, 3], B[:3, 3], Cc[:3, 3] = [1, 2, 3], [4, 5, 6], [7, 8, 9]
    B[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]          # a quarter turn about z
    c = [0.5, 0.25, 0.125]
    # expected = ((0.6 10) 10) 0.25 = 15: 12 votes score 0.8, 30 votes 1.0 (the minimum with 2), 6 votes 0.4 (cut at 0.6)
    r = ref.finish([A, B, Cc], [12, 30, 6], c, 0.6, 10, 0.6, 10)
    assert list(r["votes"]) == [30, 12] and list(r["scores"]) == [1.0, 12 / 15.0]
    assert np.array_equal(r["t"][1], [0.5, 1.75, 2.875])                   # t - c under the identity
    assert np.array_equal(r["t"][0], [4 + 0.25, 5 - 0.5, 6 - 0.125])       # t - R c
    assert np.array_equal(r["q"][1], [1, 0, 0, 0]) and np.abs(r["q"][0] - [np.sqrt(0.5), 0, 0, np.sqrt(0.5)]).max() < 1e-15
    assert len(ref.finish([A, B, Cc], [12, 30, 6], c, 0.6, 10, 0.6, 1)["votes"]) == 1        # num_result
    assert len(ref.finish([A, B, Cc], [12, 30, 6], c, 0.6, 10, 1.5, 10)["votes"]) == 0       # score_thresh above every score
    r = ref.finish([A, B, Cc], [9, 30, 9], c, 0.6, 10, 0.0, 10)                               # the sort is stable
    assert list(r["votes"]) == [30, 9, 9] and r["t"][1][0] == 0.5 and r["t"][2][0] == 6.5


# ---- the restatement against the judge and the reference's stack, on every family
@pytest.mark.parametrize("name", cu.FAMILIES)
def test_restatement_equals_the_judge(restated, name):
    j, r = cu.judged(name), restated(name)
    assert j["undecided"] == 0                                  # a condition on the inputs
    cu.assert_same_integers(r, j)
    assert all(g >= 0.1 for g in j["eigen_gaps"]), min(j["eigen_gaps"])
    if len(j["avg_poses"]):
        err = float(np.abs(r["avg_poses"] - j["avg_poses"]).max())
        print("%s: restatement against judge %.3g" % (name, err))
        assert err < 1e-13                                      # ("PPF pose clustering": the GPU tests' bar is 1e-12)


@pytest.mark.parametrize("name", cu.FAMILIES)
def test_level1_member_sets_are_the_references(restated, name):
    j, r = cu.judged(name), restated(name)
    assert cu.member_sets(r["label_t"]) == cu.reference_level1(j, cu.family(name)[1])


def test_families_are_what_they_claim(restated):
    assert cu.judged("bridge")["bridges"]                        # a non-core pose with core neighbours in two clusters
    b = restated("bridge")
    i = cu.judged("bridge")["bridges"][0]
    assert b["stats"]["clusters_t"] == 2 and b["label_t"][i] == 0      # it joins the cluster that starts first: the higher votes
    s = restated("split_rotation")
    assert (s["stats"]["clusters_t"], s["stats"]["clusters_r"]) == (1, 2)
    c = restated("chain")
    assert (c["stats"]["n_valid"], c["stats"]["clusters_t"], c["stats"]["clusters_r"]) == (300, 1, 1) and c["min_num_pt_t"] == 3
    assert int((c["count_t"] == 2).sum()) == 2 and (c["label_t"] == 0).all()
    t = restated("ties")
    assert list(t["order"]) == list(range(28)) and t["stats"]["clusters_t"] == 2 and t["cluster_votes"][0] == t["cluster_votes"][1]
    th = restated("threshold")
    assert th["stats"]["n_valid"] == 15 and th["stats"]["clusters_t"] == 1
    idn = restated("identical")
    assert idn["stats"]["clusters_t"] == 2 and sorted(idn["count_t"]) == [8] * 8 + [9] * 9
    o = restated("opposite")
    assert (o["stats"]["clusters_t"], o["stats"]["clusters_r"]) == (1, 2)
    for name in ("sparse", "single", "blobs_2"):
        assert restated(name)["stats"]["clusters_t"] == 0 and len(restated(name)["avg_votes"]) == 0
    big = restated("blobs_2049")
    assert big["stats"]["clusters_t"] >= 3 and big["stats"]["clusters_r"] > big["stats"]["clusters_t"]
    assert (big["label_t"] < 0).any() and ((big["label_t"] >= 0) & (big["count_t"] < big["min_num_pt_t"])).any()     # dropped and border poses
    for name in cu.DISTINCT_VOTES:
        assert len(set(cu.family(name)[1])) == len(cu.family(name)[1])


# ---- the header's pieces
def test_jacobi_against_eigh(ref):
    worst = 0.0
    for name in cu.FAMILIES:
        poses, votes = cu.family(name)
        r = ref.cluster(poses, votes)
        for c in range(r["stats"]["clusters_t"]):
            for s in range(int(r["label_r"][r["label_t"] == c].max()) + 1):
                who = r["order"][(r["label_t"] == c) & (r["label_r"] == s)]
                M, _, _ = ref.average(poses[who], votes[who])
                w, V = ref.jacobi4(M)
                we, Ve = np.linalg.eigh(M)
                k = int(np.argmax(w))
                assert np.abs(np.sort(w) - we).max() < 1e-13 * len(who)
                assert np.abs(V.T @ V - np.eye(4)).max() < 1e-14
                worst = max(worst, min(np.abs(V[:, k] - Ve[:, 3]).max(), np.abs(V[:, k] + Ve[:, 3]).max()))
    assert worst < 1e-14, worst
    rng = np.random.default_rng(5)
    for _ in range(200):                       # and on random symmetric matrices, repeated eigenvalues among them
        Q, _ = np.linalg.qr(rng.normal(size=(4, 4)))
        lam = rng.choice([0.0, 1.0, 2.5, -3.0, 7.0], size=4)
        M = (Q * lam) @ Q.T
        M = (M + M.T) / 2
        w, V = ref.jacobi4(M)
        assert np.abs(np.sort(w) - np.sort(lam)).max() < 1e-13 and np.abs(V @ np.diag(w) @ V.T - M).max() < 1e-13


def test_mat_to_quat_on_all_four_branches(ref):
    cases = {"tr > -1": cu.rot([1.0, 2.0, 3.0], 0.7),
             "x": cu.rot([1.0, 0.02, 0.01], np.pi - 1e-9), "y": cu.rot([0.02, 1.0, 0.01], np.pi - 1e-9),
             "z": cu.rot([0.01, 0.02, 1.0], np.pi - 1e-9)}
    # the last three: half turns (tr = -1 to rounding) forced below -1 by hand, as a pose that is a rotation to rounding can be
    seen = set()
    for name, R in cases.items():
        if name != "tr > -1":
            a = {"x": [1.0, 0, 0], "y": [0, 1.0, 0], "z": [0, 0, 1.0]}[name]
            R = 2 * np.outer(a, a) - np.eye(3)
            R = R * (1 + 2e-16)                      # tr = -1 - 2e-16: the branches for a zero scalar part
        tr = (R[0, 0] + R[1, 1]) + R[2, 2]
        branch = 0 if tr > -1 else (1 if R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2] else (2 if R[1, 1] > R[2, 2] else 3))
        seen.add(branch)
        q = ref.mat_to_quat(R)
        assert abs(np.linalg.norm(q) - 1) < 1e-15
        assert np.abs(ref.quat_to_mat(q) - R).max() < 1e-15, name
        assert np.abs(q - cu._quat_ld(R).astype(np.float64)).max() < 1e-15 or np.abs(q + cu._quat_ld(R).astype(np.float64)).max() < 1e-15
    assert seen == {0, 1, 2, 3}


def test_match_relations(ref):
    R = cu.rot([0.0, 1.0, 0.0], 0.2)
    a = cu._pose(R, [0, 0, 0])
    for ang, want in ((11.9, True), (12.1, False), (179.0, False)):
        assert ref.match(a, cu._pose(R @ cu.rot([1.0, 0, 0], ang * DEG), [0.5 * cu.R_DIST, 0, 0]), 2) is want
        assert ref.match(a, cu._pose(R @ cu.rot([1.0, 0, 0], ang * DEG), [0.5 * cu.R_DIST, 0, 0]), 1)
    assert not ref.match(a, cu._pose(R, [1.01 * cu.R_DIST, 0, 0]), 1) and not ref.match(a, cu._pose(R, [1.01 * cu.R_DIST, 0, 0]), 2)
    assert not ref.match(a, cu._pose(R, [cu.R_DIST, 0, 0]), 1)                     # d2 < r r is strict
    assert ref.match(a, a, 2, angle_threshold=1e-3)                                   # a duplicate: d2 == 0, ca within an ulp of 1
    assert ref.match(a, cu._pose(R @ cu.rot([1.0, 0, 0], np.pi), [0, 0, 0]), 2, angle_threshold=np.pi) is False   # ca = -1: acos = pi, not < pi


def test_header_stands_alone_under_sanitizers(tmp_path):
    """the restatement and the header's pieces as a stand-alone C program built with -fsanitize=address,undefined (host code)"""
    exe = str(tmp_path / "ppf_cluster_selftest")
    subprocess.run(["gcc", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "cpp", "test_ppf_cluster_fp.c"), "-o", exe, "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ---- the C ABI without a device
def test_refusals_need_no_gpu(capi):
    poses, votes = cu.family("threshold")
    bad = poses.copy()
    bad[3, 1, 2] = np.nan
    cases = [dict(poses=bad), dict(dist_threshold=0.0), dict(dist_threshold=np.inf), dict(dist_threshold=-1.0), dict(angle_threshold=0.0),
             dict(angle_threshold=3.2), dict(angle_threshold=np.nan), dict(ratio=0.0), dict(ratio=np.nan), dict(score_thresh=np.inf),
             dict(rel_dist_sparse_thresh=np.nan), dict(refine_method=7)]
    for kw in cases:
        p = kw.pop("poses", poses)
        with pytest.raises(capi.M3DError) as e:
            capi.ppf_cluster_poses(p, votes, **dict(dict(dist_threshold=cu.R_DIST), **kw))
        assert e.value.code == capi.ERR_INVALID_ARG, kw
    r = capi.ppf_cluster_poses(np.zeros((0, 4, 4)), np.zeros(0, np.uint32), dist_threshold=cu.R_DIST)      # P == 0: M3D_OK, nothing
    assert r["stats"]["n_valid"] == 0 and len(r["avg_votes"]) == 0 and len(r["order"]) == 0
    P = capi.ppf_cluster_params()
    assert (P.dist_threshold, P.ratio, P.score_thresh, P.rel_dist_sparse_thresh, P.num_result, P.refine_method) == (0.05, 0.6, 0.6, 5.0, 10, 2)
    assert P.angle_threshold == 12.0 / 180.0 * np.pi


def test_cpp_mirror_header_compiles(tmp_path):
    src = tmp_path / "use_ppf_cluster.cpp"
    src.write_text("#include <misc3d/pose_estimation/ppf_voting.h>\n"
                   "using namespace misc3d::pose_estimation;\n"
                   "size_t f(const PPFVoting& v, const double* p, size_t m, const std::vector<size_t>& r, const uint32_t* nv) {\n"
                   "    PPFClusterParams prm = v.DefaultClusterParams();\n"
                   "    prm.refine_method = RefineMethod::NoRefine;\n"
                   "    std::vector<Pose6D> out = v.Estimate(p, p, m, r, prm);\n"
                   "    PoseClusters c = v.ClusterPoses(p, nv, m, prm);\n"
                   "    return out.size() + c.avg_votes.size() + (out.empty() ? 0 : out[0].num_votes + out[0].object_id);\n}\n")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
