"""Fragment preprocessing (m3d_estimate_normals, m3d_compute_fpfh, m3d_preprocess_fragment), the part that needs no GPU: the
symbols and their argument checks, the plain-C restatement of the contract (tests/cpp/fpfh_ref.c) on inputs whose answer can
be worked out by hand and against the numpy sketch of the same contract, and the library's own pair features / bin rule
(m3d_fpfh_fp.hpp, evaluated on the host through m3d_bench_fpfh_pair_bins) against the restatement's."""
import ctypes

import numpy as np
import pytest

import fpfh_ref_util as U
import fpfh_stage_util as S


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp("fpfh_ref"))


def _row(bins, value):
    r = np.zeros(33)
    r[list(bins)] = value
    return r


def test_symbols_exported_and_bound(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in ("m3d_estimate_normals", "m3d_compute_fpfh", "m3d_preprocess_fragment", "m3d_bench_fpfh_pair_bins"):
        assert hasattr(L, name), name
        assert getattr(capi.lib(), name).argtypes, name
    for name in ("estimate_normals", "compute_fpfh_feature", "preprocess_fragment"):
        assert callable(getattr(capi, name))
    import misc3d_amd as m3d
    assert callable(m3d.features.estimate_normals) and callable(m3d.features.compute_fpfh_feature)
    assert callable(m3d.reconstruction.preprocess_fragment)


def test_argument_errors_need_no_device(capi):
    pts = np.random.default_rng(0).normal(size=(10, 3))
    nrm = np.tile([0.0, 0.0, 1.0], (10, 1))

    def err(fn, *a, **k):
        with pytest.raises(capi.M3DError) as e:
            fn(*a, **k)
        assert e.value.code == capi.ERR_INVALID_ARG
        return str(e.value)

    assert "Failed because input point cloud has no normal." in err(capi.compute_fpfh_feature, pts, None)
    for mn in (0, 129, -3):
        assert "max_nn" in err(capi.compute_fpfh_feature, pts, nrm, capi.SEARCH_HYBRID, 0.1, mn)
        assert "max_nn" in err(capi.estimate_normals, pts, capi.SEARCH_KNN, 0.0, mn)
    assert "Radius search" in err(capi.compute_fpfh_feature, pts, nrm, capi.SEARCH_RADIUS, 0.1, 30)
    assert "Radius search" in err(capi.estimate_normals, pts, capi.SEARCH_RADIUS, 0.1, 30)
    for r in (-0.1, float("nan")):
        assert "radius" in err(capi.compute_fpfh_feature, pts, nrm, capi.SEARCH_HYBRID, r, 30)
        assert "radius" in err(capi.estimate_normals, pts, capi.SEARCH_HYBRID, r, 30)
    assert "search" in err(capi.compute_fpfh_feature, pts, nrm, 7, 0.1, 30)
    for v in (0.0, -1.0, float("nan"), float("inf")):
        assert "voxel_size" in err(capi.preprocess_fragment, pts, v)
    # n == 0: success, nothing written, no device needed
    e0 = np.zeros((0, 3))
    assert capi.compute_fpfh_feature(e0, e0).shape == (0, 33)
    assert capi.estimate_normals(e0).shape == (0, 3)
    n0, f0 = capi.preprocess_fragment(e0, 0.05)
    assert n0.shape == (0, 3) and f0.shape == (0, 33)
    # n >= 2^31 is refused before the arrays are read
    L = capi.lib()
    assert L.m3d_compute_fpfh(pts.ctypes.data, nrm.ctypes.data, 2**31, 2, 0.1, 30, 0, pts.ctypes.data, None) == capi.ERR_INVALID_ARG
    assert "2^31" in capi.last_error()
    assert L.m3d_estimate_normals(pts.ctypes.data, 2**31, 2, 0.1, 30, 0, None, 0, pts.ctypes.data, None) == capi.ERR_INVALID_ARG


def test_python_layer_errors(capi):
    import misc3d_amd as m3d
    pts = np.zeros((5, 3))
    with pytest.raises(RuntimeError, match="no normal"):
        m3d.features.compute_fpfh_feature(pts, ("hybrid", 0.1, 100))
    with pytest.raises(RuntimeError, match="Radius search"):
        m3d.features.estimate_normals(pts, ("radius", 0.1))
    with pytest.raises(RuntimeError, match="max_nn"):
        m3d.features.compute_fpfh_feature((pts, pts), ("knn", 129))


def test_restatement_two_points_by_hand(ref):
    # both normals (0, 0, 1), the pair along x: a1 = a2 = 0, v = (0, -1, 0), w = (1, 0, 0), f = (atan2(0, 1), 0, 0) = 0:
    # bins floor(5.5) = 5, 11 + 5, 22 + 5; m = 2 -> incr = 100; FPFH = 100 / 1 * (100 / 100) + 100 = 200
    pts = np.array([[0.0, 0, 0], [1.0, 0, 0]])
    nrm = np.array([[0.0, 0, 1], [0.0, 0, 1]])
    out, spfh = ref.fpfh(pts, nrm, U.KNN, 0.0, 2, spfh=True)
    assert np.array_equal(spfh, np.stack([_row((5, 16, 27), 100.0)] * 2))
    assert np.array_equal(out, np.stack([_row((5, 16, 27), 200.0)] * 2))
    # n2 = (0.6, 0, 0.8).  From point 0: a1 = 0, a2 = 0.6, acos(0) > acos(0.6): swap, dp = (-1, 0, 0), f2 = -0.6,
    # v = dp x n2 = (0, 0.8, 0) -> (0, 1, 0), w = n2 x v = (-0.8, 0, 0.6), f1 = v . n1 = 0, f0 = atan2(0.6, 0.8) = 0.6435:
    # bins floor(11 (0.6435 + pi) / (2 pi)) = floor(6.63) = 6, 11 + floor(5.5) = 16, 22 + floor(11 * 0.4 / 2) = 22 + 2.
    # From point 1: dp = (-1, 0, 0), a1 = -0.6, a2 = 0, acos(0.6) < acos(0): no swap, the same frame: the same bins.
    nrm = np.array([[0.0, 0, 1], [0.6, 0, 0.8]])
    bins, feat = ref.pair_bins(np.concatenate([pts[0], nrm[0], pts[1], nrm[1]])[None, :])
    assert bins.tolist() == [[6, 16, 24]]
    assert np.allclose(feat[0], [np.arctan2(0.6, 0.8), 0.0, -0.6], rtol=0, atol=1e-15)
    out, spfh = ref.fpfh(pts, nrm, U.KNN, 0.0, 2, spfh=True)
    assert np.array_equal(spfh, np.stack([_row((6, 16, 24), 100.0)] * 2))
    assert np.array_equal(out, np.stack([_row((6, 16, 24), 200.0)] * 2))


def test_restatement_exact_plane(ref):
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.uniform(-1, 1, size=(600, 2)), np.zeros((600, 1))], 1)
    pts = np.concatenate([pts, [[50.0, 50.0, 0.0]]])          # + one isolated point
    nrm = np.tile([0.0, 0.0, 1.0], (len(pts), 1))
    out = ref.fpfh(pts, nrm, U.HYBRID, 0.2, 100)
    _, _, m = ref.neighbours(pts, U.HYBRID, 0.2, 100)
    assert m[-1] == 1 and (m[:-1] > 1).all()
    assert np.allclose(out[:-1], _row((5, 16, 27), 200.0), rtol=0, atol=1e-9)
    assert not out[-1].any()                                   # the isolated point: a zero row


def test_restatement_duplicates(ref):
    # A twice (indices 0, 1), B once: the lists are ordered by (d2, index), so point 1's entry 0 is point 0 and the point
    # itself comes at k = 1 with d = 0 (features 0 -> bins 5, 16, 27) and d2 = 0 (skipped by the FPFH weights)
    pts = np.array([[0.0, 0, 0], [0.0, 0, 0], [1.0, 0, 0]])
    nrm = np.tile([0.0, 0.0, 1.0], (3, 1))
    idx, d2, m = ref.neighbours(pts, U.KNN, 0.0, 3)
    assert idx.tolist() == [[0, 1, 2], [0, 1, 2], [2, 0, 1]] and m.tolist() == [3, 3, 3]
    out, spfh = ref.fpfh(pts, nrm, U.KNN, 0.0, 3, spfh=True)
    assert np.array_equal(spfh, np.stack([_row((5, 16, 27), 100.0)] * 3))
    assert np.array_equal(out, np.stack([_row((5, 16, 27), 200.0)] * 3))
    assert np.isfinite(out).all()
    # a NaN point has no neighbours and is nobody's neighbour
    pts2 = np.concatenate([pts, [[np.nan, 0, 0]]])
    nrm2 = np.tile([0.0, 0.0, 1.0], (4, 1))
    out2 = ref.fpfh(pts2, nrm2, U.KNN, 0.0, 3)
    assert np.array_equal(out2[:3], out) and not out2[3].any()


def test_restatement_equals_numpy_sketch(ref):
    pts, nrm = U.three_surface_cloud(4000, seed=5)
    for search, radius, k in ((U.HYBRID, 0.2, 100), (U.HYBRID, 0.1, 30), (U.KNN, 0.0, 30), (U.KNN, 0.0, 128)):
        a = ref.fpfh(pts, nrm, search, radius, k)
        b = U.np_fpfh(pts, nrm, search, radius, k)
        assert len(U.differing_points(a, b)) == 0, (search, radius, k, np.abs(a - b).max())
        assert U.group_sums_ok(a).all()
    # neighbour choice through equal distances: (d2, index)
    lat = U.lattice(6)
    idx, d2, m = ref.neighbours(lat, U.KNN, 0.0, 5)
    ii, dd, _ = U.np_neighbours(lat, U.KNN, 0.0, 5)
    assert np.array_equal(idx, ii) and np.array_equal(d2, dd)


def test_restatement_normals(ref):
    pts, _ = U.three_surface_cloud(3000, seed=6)
    got = ref.normals(pts, U.HYBRID, 0.2, 30)
    idx, _, m = ref.neighbours(pts, U.HYBRID, 0.2, 30)
    want, gap = U.np_normals(pts, idx, m)
    ok = gap >= 1e-2
    assert ok.mean() >= 0.99
    assert np.linalg.norm(np.cross(got[ok], want[ok]), axis=1).max() <= 1e-8
    o = ref.normals(pts, U.HYBRID, 0.2, 30, orient_to=(0, 0, 0))
    assert ((o * (0 - pts)).sum(1) >= 0).all() and np.array_equal(np.abs(o), np.abs(got))


def test_host_evaluator_matches_restatement_bins(capi, ref):
    rng = np.random.default_rng(17)
    m = 100_000
    p1 = rng.normal(size=(m, 3))
    p2 = p1 + rng.normal(size=(m, 3)) * rng.choice([1e-3, 0.05, 1.0], size=(m, 1))
    n1 = rng.normal(size=(m, 3))
    n2 = rng.normal(size=(m, 3))
    n1 /= np.linalg.norm(n1, axis=1, keepdims=True)
    n2 /= np.linalg.norm(n2, axis=1, keepdims=True)
    n2[:1000] = n1[:1000]                                       # parallel normals
    p2[1000:1100] = p1[1000:1100]                               # coincident points
    n1[1100:1200] = (p2[1100:1200] - p1[1100:1200]) / np.linalg.norm(p2[1100:1200] - p1[1100:1200], axis=1, keepdims=True)
    pairs = np.concatenate([p1, n1, p2, n2], 1)
    got, gf = capi.fpfh_pair_bins(pairs, features=True)
    want, wf = ref.pair_bins(pairs)
    if capi.FP_ORDER == 1:     # e0 + (e1 + e2): features within roundings, a bin may move where its coordinate is an integer
        assert np.allclose(gf, wf, rtol=0, atol=1e-9) and (got != want).any(1).mean() < 1e-3
    else:
        assert np.array_equal(got, want)
        assert np.array_equal(gf, wf)
    assert (got[:, 0] >= 0).all() and (got[:, 0] <= 10).all() and (got[:, 1] >= 11).all() and (got[:, 2] <= 32).all()
    assert (got[1000:1100] == [5, 16, 27]).all()


# ---- the stage references (tests/fpfh_stage_util.py) held to the restatement -------------------------------------------------
def _sketch_inputs():
    pts, nrm = U.three_surface_cloud(4000, seed=5)
    return [S._case(f"sketch_{s}_{r}_{k}", pts, nrm, s, r, k)
            for s, r, k in ((U.HYBRID, 0.2, 100), (U.HYBRID, 0.1, 30), (U.KNN, 0.0, 30), (U.KNN, 0.0, 128))]


def test_stage_references_match_restatement(ref):
    for c in _sketch_inputs() + list(S.seam_cases().values()):
        pts, nrm, a = c["pts"], c["nrm"], (c["search"], c["radius"], c["k"])
        want, sp = ref.fpfh(pts, nrm, *a, spfh=True)
        lists = ref.neighbours(pts, *a)
        counts, m = S.ref_counts(ref, pts, nrm, *a, lists=lists)
        incr = S.incr_of(m)
        assert np.allclose(counts * incr[:, None], sp, rtol=0, atol=1e-9), c["name"]
        with np.errstate(invalid="ignore", divide="ignore"):
            back = np.where(incr[:, None] != 0, np.rint(sp / incr[:, None]), 0.0)
        assert np.array_equal(back, counts), c["name"]
        assert (counts.sum(1) == 3 * np.maximum(m - 1, 0)).all() and counts.max(initial=0) <= 127, c["name"]
        got = S.assemble(lists[0], lists[1], m, counts, incr)
        assert len(U.differing_points(got, want)) == 0, (c["name"], np.abs(got - want).max())


def test_stage_inputs_have_no_undecided_pair(ref):
    """every input of tests/test_gpu_fpfh_stages.py: no pair within 1e-9 of a bin edge (so the device's counts must equal the
    restatement's on every point), and the points inside the 32 / 64 / 128 eps tie bands, pinned"""
    cases = {**S.seam_cases(), **S.big_cases(), **S.tie_cases(ref)}
    ties = {}
    for name, c in cases.items():
        r = S.reference(ref, c)
        n_und = len(np.unique(r["own"][r["undecided"]]))
        t = tuple(int(b.sum()) for b in r["bands"])
        print(f"{name}: n={len(c['pts'])} pairs={len(r['own'])} undecided pairs={int(r['undecided'].sum())} points={n_und} "
              f"tie points (32, 64, 128 eps)={t}")
        assert n_und == 0, name
        assert (r["bands"][0] <= r["bands"][1]).all() and (r["bands"][1] <= r["bands"][2]).all()
        if any(t):
            ties[name] = t
    assert ties == S.TIE_COUNTS
    assert ties["tie6000"][0] > 64 and ties["tie1500"][0] > 0       # more than one block of fpfh_tie_scatter_k; a strided gather
