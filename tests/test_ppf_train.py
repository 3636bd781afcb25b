"""The PPF model preprocessing without a GPU: the contract's restatement (tests/cpp/ppf_train_ref.c, the reference's heap walk
and FIFO sampler) on hand cases and against an independent judge (Kruskal under O2, a breadth-first pass, scipy's spanning tree)
on every input family of the GPU test; the library's host steps (m3d_ppf_train.hpp compiled alone with g++) against the
restatement byte for byte; SampleWithoutDuplicate against std::mt19937; the config classes and the C++ mirror; and the restatement
chain end to end on the two scenes of tests/test_gpu_ppf_estimator.py, inside that test's bar."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ppf_edge_ref_util as eu
import ppf_train_ref_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_p = tu._p


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tu.TrainRef(tmp_path_factory.mktemp("ppf_train_ref"))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """m3d_ppf_train.hpp alone under g++ (tests/cpp/ppf_train_host.cpp)"""
    so = str(tmp_path_factory.mktemp("ppf_train_host") / "ppf_train_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "cpp", "ppf_train_host.cpp"),
                    "-o", so], check=True)
    L = C.CDLL(so)
    L.pth_sample.restype = C.c_size_t
    L.pth_sample.argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_size_t, C.c_void_p, C.c_void_p]
    L.pth_tree_signs.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pth_box.restype = None
    L.pth_box.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.pth_derive.restype = None
    L.pth_derive.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p]
    L.pth_seed.restype = C.c_size_t
    L.pth_seed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
    L.pth_reference_indices.restype = None
    L.pth_reference_indices.argtypes = [C.c_size_t, C.c_size_t, C.c_uint32, C.c_void_p]
    return L


def _host_sample(host, pts, step, seed):
    pts = tu._f(pts)
    out, ev = np.zeros(len(pts), np.uint64), np.zeros(1, np.uint64)
    k = host.pth_sample(_p(pts), len(pts), float(step), int(seed), _p(out), _p(ev))
    return out[:k].astype(np.int64), int(ev[0])


# ---- the orientation: hand cases
def test_orient_hand_cases(ref):
    up, down = [0.0, 0.0, 1.0], [0.0, 0.0, -2.0]
    n, p, st = ref.orient([[1.0, 2.0, 3.0]], [down], 0.5, 0)                        # the seed alone: never flipped
    assert n.tolist() == [down] and p.tolist() == [-1] and st == dict(rounds=1, tree_edges=0, component=1, flips=0)
    n, p, st = ref.orient([[0.0, 0, 0], [0.5, 0, 0]], [up, down], 1.0, 1)           # two points, the seed is the second
    assert n.tolist() == [[0.0, 0.0, -1.0], down] and p.tolist() == [1, -1] and st["flips"] == 1 and st["tree_edges"] == 1
    n, p, st = ref.orient([[0.0, 0, 0], [0.5, 0, 0]], [up, down], 0.5, 1)           # d2 == radius^2 is no edge
    assert n.tolist() == [up, down] and p.tolist() == [-2, -1] and st["component"] == 1 and st["tree_edges"] == 0
    # the seed pushes 1 (0.36) and 2 (0.81); 1 is popped first and pushes 2 again with 0.09: 2's parent is 1, not the seed
    n, p, st = ref.orient([[0.0, 0, 0], [0.6, 0, 0], [0.9, 0, 0]], [up, down, down], 1.0, 0)
    assert p.tolist() == [-1, 0, 1] and n.tolist() == [up, [0.0, 0.0, 2.0], [0.0, 0.0, 2.0]] and st["flips"] == 2
    # a zero dot resets the sign: 1 is flipped (s = -1), 2 is perpendicular to 1 and stays whatever 1's sign, 3 follows 2
    pts = [[0.0, 0, 0], [0.6, 0, 0], [1.2, 0, 0], [1.8, 0, 0]]
    n, p, st = ref.orient(pts, [up, down, [1.0, 0, 0], [-1.0, 0, 0]], 0.7, 0)
    assert p.tolist() == [-1, 0, 1, 2] and n.tolist() == [up, [0.0, 0.0, 2.0], [1.0, 0, 0], [1.0, 0, 0]] and st["flips"] == 2
    n, p, st = ref.orient(pts, [up, down, [np.nan, 0, 0], [-1.0, 0, 0]], 0.7, 0)    # a NaN dot flips nothing either
    assert p.tolist() == [-1, 0, 1, 2] and st["flips"] == 1 and n[3].tolist() == [-1.0, 0, 0]


# ---- the restatement against the judge on every family of the GPU test
@pytest.mark.parametrize("name", tu.ORIENT_CASES)
def test_heap_walk_equals_kruskal(ref, host, name):
    c = tu.orient_case(name)
    n, p, st = ref.orient(**c)
    jn, jp, jst, tree = tu.judge_orient(**c)
    assert np.array_equal(p, jp) and n.tobytes() == jn.tobytes()
    assert {k: st[k] for k in jst} == jst
    # the library's tree-to-signs pass (m3d_ppf_train.hpp under g++) on the judge's tree, its edges in a shuffled order
    edges = np.array(sorted(tree), dtype=np.uint32).reshape(-1, 2)
    edges = np.ascontiguousarray(edges[np.random.default_rng(1).permutation(len(edges))])
    out, parent, counts = np.zeros_like(n), np.zeros(len(p), np.int64), np.zeros(2, np.uint64)
    nrm = tu._f(c["normals"])
    assert host.pth_tree_signs(_p(edges), len(edges), _p(nrm), len(nrm), c["seed"], _p(out), _p(parent), _p(counts)) == 1
    assert np.array_equal(parent, p) and out.tobytes() == n.tobytes() and counts.tolist() == [st["component"], st["flips"]]
    if name in tu.TIE_FREE:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import minimum_spanning_tree
        e = tu.radius_edges(c["points"], c["radius"])
        assert len({d2 for d2, _, _ in e}) == len(e) and min(d2 for d2, _, _ in e) > 0      # tie-free, and no zero weight
        g = coo_matrix(([d2 for d2, _, _ in e], ([lo for _, lo, _ in e], [hi for _, _, hi in e])), shape=(len(p), len(p)))
        t = minimum_spanning_tree(g.tocsr()).tocoo()
        assert {(min(a, b), max(a, b)) for a, b in zip(t.row.tolist(), t.col.tolist())} == tree


def test_tree_signs_refuses_an_index_outside_the_cloud(host):
    edges = np.array([[0, 5]], dtype=np.uint32)
    nrm, out, parent, counts = np.ones((3, 3)), np.zeros((3, 3)), np.zeros(3, np.int64), np.zeros(2, np.uint64)
    assert host.pth_tree_signs(_p(edges), 1, _p(nrm), 3, 0, _p(out), _p(parent), _p(counts)) == 0


# ---- the sampler
def test_sampler_on_a_line(ref, host):
    """20 points spaced 1, step 2.5: a point is selected, its neighbours closer than 2.5 are struck out, those in [2.5, 5) are
    queued -- 5 itself is not a neighbour (d2 < (2 step)^2 is strict) -- so every third point is selected"""
    pts = np.zeros((20, 3))
    pts[:, 0] = np.arange(20.0)
    assert ref.sample(pts, 2.5, 0).tolist() == [0, 3, 6, 9, 12, 15, 18]
    assert _host_sample(host, pts, 2.5, 0)[0].tolist() == [0, 3, 6, 9, 12, 15, 18]
    assert ref.sample(pts, 2.5, 10).tolist() == [10, 7, 13, 4, 16, 1, 19]      # both ways from the middle, the lower index first
    assert _host_sample(host, pts, 2.5, 10)[0].tolist() == [10, 7, 13, 4, 16, 1, 19]
    assert ref.sample(pts, 0.4, 4).tolist() == [4]                                # nothing within 2 step: the seed alone


@pytest.fixture(scope="module")
def clouds():
    pts, _, _, _, _ = eu.plate_with_holes(n_side=60, seed=11)
    g = np.load(os.path.join(ROOT, "tests", "golden", "raycast_obj.npz"))
    rng = np.random.default_rng(4)
    lattice = np.stack(np.meshgrid(np.arange(12.0), np.arange(12.0), np.arange(3.0), indexing="ij"), axis=-1).reshape(-1, 3)
    return dict(plate=np.ascontiguousarray(pts + np.array([0.1, -0.2, 1.5])), obj=np.ascontiguousarray(g["vertices"].astype(np.float64) * 0.001),
                random=rng.uniform(-1, 1, size=(1500, 3)), lattice=np.ascontiguousarray(lattice[rng.permutation(len(lattice))]))


@pytest.mark.parametrize("name", ("plate", "obj", "random", "lattice"))
def test_host_steps_equal_the_restatement(ref, host, clouds, name):
    pts = clouds[name]
    c, e = ref.box(pts)
    hc, he = np.zeros(3), np.zeros(3)
    host.pth_box(_p(pts), len(pts), _p(hc), _p(he))
    assert hc.tobytes() == c.tobytes() and he.tobytes() == e.tobytes()
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    assert (e > 0).all() and np.linalg.norm(e) <= np.linalg.norm(hi - lo) * np.sqrt(3) and (c > lo - 1e-9).all() and (c < hi + 1e-9).all()
    d = ref.derive(c, e)
    o = np.zeros(8)
    host.pth_derive(_p(c), _p(e), 0.05, 0.025, 0.01, _p(o))
    assert o.tobytes() == np.array([d["diameter"], d["r_min"], d["dist_step"], d["dist_step_dense"], d["normal_r"], *d["view_pt"]]).tobytes()
    assert d["r_min"] == np.sqrt(np.sort(e)[0] ** 2 + np.sort(e)[1] ** 2) and d["view_pt"][2] == c[2] + 2.0 * d["diameter"]
    rng = np.random.default_rng(2)
    nrm = np.ascontiguousarray(rng.normal(size=pts.shape))
    for invert in (0, 1):
        r = ref.prepare_model(pts, nrm, box=(c, e), rel_dense_sample_dist=0.0, keep_normals=False, invert_model_normal=bool(invert),
                              calc_normal_relative=1e-9)["info"]        # (a radius that isolates the seed: B3 and B4 alone)
        unit = nrm / np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])[:, None]
        flips = C.c_int(-1)
        seed = host.pth_seed(_p(pts), _p(np.ascontiguousarray(unit)), len(pts), _p(d["view_pt"]), invert, C.byref(flips))
        assert (seed, flips.value) == (r["seed"], r["seed_flipped"])
        assert seed == int(np.argmin(((pts - d["view_pt"]) ** 2).sum(axis=1)))
    for step in (d["dist_step"], d["dist_step_dense"], 3.0 * d["dist_step"]):
        want = ref.sample(pts, step, seed)
        got, evals = _host_sample(host, pts, step, seed)
        assert np.array_equal(got, want) and len(set(got.tolist())) == len(got) and got[0] == seed
        assert len(got) <= evals <= len(got) * len(pts)
        # no two selected points are closer than the step
        sel = pts[got]
        d2 = ((sel[:, None, :] - sel[None, :, :]) ** 2).sum(axis=2) + np.eye(len(sel)) * 1e9
        assert np.sqrt(d2.min()) >= step * (1 - 1e-12)


# ---- SampleWithoutDuplicate
STD_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>
int main(int, char** a) {
    const size_t size = std::strtoull(a[1], 0, 10), sample = std::strtoull(a[2], 0, 10);
    std::mt19937 rng((unsigned)std::strtoul(a[3], 0, 10));
    std::vector<size_t> indices(size);
    std::iota(indices.begin(), indices.end(), 0);
    for (size_t i = 0; i < sample; ++i) std::swap(indices[i], indices[rng() % size]);
    for (size_t i = 0; i < sample; ++i) std::printf("%zu\n", indices[i]);
}
"""


def test_reference_indices_are_the_standard_librarys(capi, ref, host, tmp_path):
    src, exe = tmp_path / "swd.cpp", str(tmp_path / "swd")
    src.write_text(STD_PROGRAM)
    subprocess.run(["g++", "-O1", "-std=c++17", str(src), "-o", exe], check=True)
    for num, sample, seed in ((10, 6, 7), (1000, 600, 123456789), (3, 3, 0), (2497, 1498, 4294967295)):
        want = np.array(subprocess.run([exe, str(num), str(sample), str(seed)], capture_output=True, text=True, check=True).stdout.split(),
                        dtype=np.int64)
        assert np.array_equal(capi.ppf_reference_indices(num, sample, seed), want)
        assert np.array_equal(ref.reference_indices(num, sample, seed), want)
        out = np.zeros(sample, np.uint64)
        host.pth_reference_indices(num, sample, seed, _p(out))
        assert np.array_equal(out.astype(np.int64), want) and len(set(want.tolist())) == sample
    assert len(capi.ppf_reference_indices(5, 0, 1)) == 0
    for num, sample in ((5, 6), (0, 0), (2 ** 32, 1)):
        with pytest.raises(capi.M3DError):
            capi.ppf_reference_indices(num, sample, 1)


# ---- the classes
def test_config_defaults_and_check_config(capi):
    import misc3d_amd as m3d
    pe = m3d.pose_estimation
    c = pe.PPFEstimatorConfig()
    t, v = c.training_param, c.voting_param
    assert (t.invert_model_normal, t.use_external_normal, t.rel_sample_dist, t.rel_dense_sample_dist, t.calc_normal_relative) == (False, False, 0.05, 0.025, 0.01)
    assert (c.ref_param.method, c.ref_param.ratio) == (pe.PPFEstimatorConfig.ReferencePointSelection.Random, 0.6)
    assert (v.method, v.faster_mode, v.angle_step, v.min_dist_thresh, v.min_angle_thresh) == (
        pe.PPFEstimatorConfig.VotingMode.SampledPoints, True, 12.0 / 180 * np.pi, 1.0 / 3, 30.0 / 180 * np.pi)
    assert c.edge_param.pts_num == 20 and (c.refine_param.method, c.refine_param.rel_dist_sparse_thresh) == (pe.PPFEstimatorConfig.PointToPlane, 5)
    assert (c.rel_dist_thresh, c.rel_angle_thresh, c.score_thresh, c.num_result, c.object_id) == (0.05, 12.0 / 180 * np.pi, 0.6, 10, 0)
    assert pe.PPFEstimatorConfig.RefineMethod.PointToPlane is pe.PPFEstimatorConfig.PointToPlane and pe.PPFEstimatorConfig.EdgePoints.name == "EdgePoints"
    P = capi.ppf_train_params()
    assert (P.rel_sample_dist, P.rel_dense_sample_dist, P.calc_normal_relative, P.invert_model_normal, P.use_external_normal, P.pts_num) == (
        0.05, 0.025, 0.01, 0, 0, 20)
    with pytest.raises(TypeError):
        capi.ppf_train_params(no_such_field=1)
    est = pe.PPFEstimator(c)
    assert est.estimate(np.zeros((5, 3))) == (False, []) and est.get_pose() == [] and est.getl_pose() == []     # not trained
    assert est.train(np.zeros((0, 3))) is False and est.get_model_diameter() == 0.0
    assert all(a.shape == (0, 3) for pair in (est.get_sampled_model(), est.get_sampled_scene(), est.get_model_edges(), est.get_scene_edges())
               for a in pair)
    c.training_param.rel_dense_sample_dist = 0.05                 # dense >= sparse
    assert pe.PPFEstimator.check_config(c) is False and est.set_config(c) is False
    with pytest.raises(ValueError):
        pe.PPFEstimator(c)
    c.training_param.rel_dense_sample_dist = 0.049
    assert est.set_config(c) is True


def test_argument_checks_need_no_gpu(capi):
    pts, nrm = np.zeros((4, 3)), np.ones((4, 3))
    with pytest.raises(capi.M3DError, match="radius"):
        capi.orient_normals_mst(pts, nrm, 0.0, 0)
    with pytest.raises(capi.M3DError, match="seed"):
        capi.orient_normals_mst(pts, nrm, 1.0, 4)
    with pytest.raises(capi.M3DError, match="no points"):
        capi.orient_normals_mst(np.zeros((0, 3)), np.zeros((0, 3)), 1.0, 0)
    pts[2, 0] = np.inf
    with pytest.raises(capi.M3DError, match="point 2 is not finite"):
        capi.orient_normals_mst(pts, nrm, 1.0, 0)
    with pytest.raises(capi.M3DError, match="point 2 is not finite"):
        capi.ppf_prepare_model(pts)
    with pytest.raises(capi.M3DError, match="There is no input points"):
        capi.ppf_prepare_model(np.zeros((0, 3)))
    with pytest.raises(ValueError):
        capi.ppf_prepare_model(np.zeros((4, 3)), box_center=[0, 0, 0])


# ---- the restatement chain end to end on the scenes of tests/test_gpu_ppf_estimator.py: the inputs themselves meet that test's bar
@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    import ppf_estimator_scene_util as su
    return su.Chain(tmp_path_factory.mktemp("ppf_estimator_chain"))


def test_restatement_chain_on_the_reference_examples_shape(chain):
    """train (ppf_train_ref.c on the restated normals), the scene prepared by the restatements, ppf_ref.c, ppf_cluster_ref.c with the
    ICP restatement: the top pose within one dist_step and one angle_step of the rendering pose -- the quantisation of the vote"""
    import ppf_estimator_scene_util as su
    meshes, poses, cam, T = su.obj_scene_meshes()
    scene = su.cloud_of(chain.render(meshes, poses, cam)["t_hit"], cam)
    res, info, counts = chain.run(np.ascontiguousarray(meshes[0][0]), None, scene, None, su.OBJ_NORMAL_REL, False, 0.01)
    assert len(res["votes"]) >= 1
    dt, dr = su.pose_error(res["poses"][0], T)
    print(counts, "votes", list(res["votes"]), "scores", list(res["scores"]), "translation error", dt, "of dist_step", info["dist_step"],
          "rotation error", dr, "of angle_step", 12.0 / 180 * np.pi)
    assert dt <= info["dist_step"] and dr <= 12.0 / 180 * np.pi


def test_restatement_chain_in_edge_points_mode(chain):
    import ppf_estimator_scene_util as su
    model, nrm = su.plate_model()
    m = chain.train.prepare_model(model, nrm, calc_normal_relative=su.PLATE_NORMAL_REL)
    sp, sn, T = su.plate_scene(model, m["normals"])
    res, info, counts = chain.run(model, nrm, sp, sn, su.PLATE_NORMAL_REL, True, 0.0)
    assert len(res["votes"]) >= 1 and 0 < counts["model_edges"] < counts["model_dense"] // 2      # rims and holes, not faces
    dt, dr = su.pose_error(res["poses"][0], T)
    print(counts, "votes", list(res["votes"])[:3], "translation error", dt, "of dist_step", info["dist_step"], "rotation error", dr,
          "of angle_step", 12.0 / 180 * np.pi)
    assert dt <= info["dist_step"] and dr <= 12.0 / 180 * np.pi


def test_exported_symbols(capi):
    L = C.CDLL(capi.LIB_PATH)
    for name in ("m3d_orient_normals_mst", "m3d_ppf_prepare_model", "m3d_ppf_reference_indices", "m3d_ppf_train_params_default_"):
        assert hasattr(L, name), name
    assert C.sizeof(capi.OrientStats) == 64 and C.sizeof(capi.PpfTrainParams) == 40 and C.sizeof(capi.PpfModelInfo) == 256


def test_cpp_mirror(tmp_path):
    exe = str(tmp_path / "test_ppf_estimator_mirror")
    lib = os.path.join(ROOT, "misc3d_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_ppf_estimator_mirror.cpp"),
                    "-o", exe, "-L", lib, "-lmisc3d_amd", "-lpthread", "-Wl,-rpath," + lib], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
