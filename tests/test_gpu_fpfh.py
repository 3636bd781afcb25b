"""Fragment preprocessing on the device against the plain-C restatement of the contract (tests/cpp/fpfh_ref.c), through the C
ABI (capi) and through the python API.

FPFH rows are compared with rtol = atol = 1e-9.  The one legitimate cause of a larger difference is a pair whose bin
coordinate lies within a few ulp of an integer, so that the device's atan2 / division rounds to the other side: at most
0.1 % of the points may differ, and every row must keep its group sums (200 / 100 / 0 within 1e-9).  The number of differing
points is printed.  Normals are compared by direction (|n_gpu x n_ref| <= 1e-8) with numpy's eigh on the centred covariance of
the restatement's neighbour sets, on the points whose relative eigenvalue gap is >= 1e-2 (at most 1 % excluded).

Oriented normals: the contract negates a normal when n . (camera - p) < 0, the (0, 0, 1) of a point with m < 3 included, so
"(0, 0, 1) where m < 3" is asserted on the call without orientation and (0, 0, +-1) plus the orientation condition on the
call with it.

Estimated normals of neighbouring points often come from the same neighbours and agree to an ulp; the contract's
acos(|a1|) > acos(|a2|) is then a near tie that two libms may order differently (it swaps the pair's frame: other bins, and the
row reaches every point that has it in its list).  The library lets the host decide those rows (m3d_fpfh_stats.tie_points);
test_end_to_end_registration, whose normals are estimated, is the test that needs it."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import fpfh_ref_util as U

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CAP = 1e-3          # fraction of points that may differ (bin coordinates on an integer)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp("fpfh_ref"))


@pytest.fixture(scope="module")
def cloud():
    return U.three_surface_cloud(20000)


def _compare(got, want, what, defer=None):
    bad = U.differing_points(got, want)
    print(f"{what}: {len(bad)} of {len(want)} points differ (cap {int(CAP * len(want))})")
    if defer is not None:      # asserted by the caller at the end of its test, so that its other checks run first
        defer.append((what, len(bad), len(want)))
    else:
        assert len(bad) <= CAP * len(want), (what, len(bad))
    assert U.group_sums_ok(got).all(), what
    return bad


def _row(bins, value):
    r = np.zeros(33)
    r[list(bins)] = value
    return r


@pytest.mark.parametrize("search,radius,k", [(U.HYBRID, 0.1, 100), (U.HYBRID, 0.05, 30), (U.KNN, 0.0, 30), (U.KNN, 0.0, 128)])
def test_fpfh_matches_restatement(capi, ref, cloud, search, radius, k):
    import misc3d_amd as m3d
    pts, nrm = cloud
    want = ref.fpfh(pts, nrm, search, radius, k)
    got, st = capi.compute_fpfh_feature(pts, nrm, search, radius, k, stats=True)
    _compare(got, want, f"fpfh search={search} radius={radius} max_nn={k}")
    _, _, m = ref.neighbours(pts, search, radius, k)
    assert st["pairs"] == int(m.sum()) and st["searches"] == 1 and st["launches"] >= 4 and st["ms_device"] > 0
    param = ("hybrid", radius, k) if search == U.HYBRID else ("knn", k)
    py = m3d.features.compute_fpfh_feature((pts, nrm), param)
    assert py.shape == (33, len(pts)) and np.array_equal(py.T, got)


def test_fpfh_under_alternative_associations(ref, tmp_path):
    pts, nrm = U.three_surface_cloud(5000, seed=12)
    want = ref.fpfh(pts, nrm, U.HYBRID, 0.2, 100)
    np.save(tmp_path / "pts.npy", pts)
    np.save(tmp_path / "nrm.npy", nrm)
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1]); from misc3d_amd import capi; d = sys.argv[2];"
            "np.save(d + '/out.npy', capi.compute_fpfh_feature(np.load(d + '/pts.npy'), np.load(d + '/nrm.npy'), 2, 0.2, 100))")
    for order in (1, 2):
        env = dict(os.environ, M3D_FP_ORDER=str(order))
        p = subprocess.run([sys.executable, "-c", code, ROOT, str(tmp_path)], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-2000:]
        _compare(np.load(tmp_path / "out.npy"), want, f"fpfh order{order}")


def test_exact_cases(capi, ref):
    rng = np.random.default_rng(3)
    pl = np.concatenate([rng.uniform(-1, 1, size=(600, 2)), np.zeros((600, 1))], 1)
    pts = np.concatenate([pl, [[50.0, 50.0, 0.0]]])                       # the plane z = 0 + an isolated point
    nrm = np.tile([0.0, 0.0, 1.0], (len(pts), 1))
    out = capi.compute_fpfh_feature(pts, nrm, U.HYBRID, 0.2, 100)
    assert np.allclose(out[:-1], _row((5, 16, 27), 200.0), rtol=0, atol=1e-9) and not out[-1].any()
    # duplicates: d == 0 pairs and d2 == 0 weights
    dup = np.array([[0.0, 0, 0], [0.0, 0, 0], [1.0, 0, 0]])
    dn = np.tile([0.0, 0.0, 1.0], (3, 1))
    out = capi.compute_fpfh_feature(dup, dn, U.KNN, 0.0, 3)
    assert np.allclose(out, _row((5, 16, 27), 200.0), rtol=0, atol=1e-9)
    cl, cn = U.three_surface_cloud(2000, seed=4)
    cl[100] = cl[7]
    cl[101] = cl[7]
    _compare(capi.compute_fpfh_feature(cl, cn, U.HYBRID, 0.2, 50), ref.fpfh(cl, cn, U.HYBRID, 0.2, 50), "duplicates")
    # a NaN point: a zero row, and no other row changes when it is removed
    base = capi.compute_fpfh_feature(cl, cn, U.HYBRID, 0.2, 50)
    cl2 = np.concatenate([cl[:500], [[np.nan, 1.0, 2.0]], cl[500:], [[0.0, np.inf, 0.0]]])
    cn2 = np.concatenate([cn[:500], [[0.0, 0, 1]], cn[500:], [[0.0, 0, 1]]])
    out = capi.compute_fpfh_feature(cl2, cn2, U.HYBRID, 0.2, 50)
    assert not out[500].any() and not out[-1].any()
    assert np.array_equal(np.concatenate([out[:500], out[501:-1]]), base)
    nn = capi.estimate_normals(cl2, U.HYBRID, 0.2, 30)
    assert np.array_equal(nn[500], [0, 0, 1]) and np.array_equal(nn[-1], [0, 0, 1])
    # tiny clouds
    for n in (1, 2, 3, 64, 65):
        p, q = U.three_surface_cloud(max(n, 3), seed=n)
        p, q = p[:n], q[:n]
        for search, radius, k in ((U.KNN, 0.0, 30), (U.HYBRID, 10.0, 100), (U.KNN, 0.0, 1)):
            got = capi.compute_fpfh_feature(p, q, search, radius, k)
            bad = U.differing_points(got, ref.fpfh(p, q, search, radius, k))
            assert len(bad) == 0 and U.group_sums_ok(got).all(), (n, search, k)
        assert np.allclose(np.abs((capi.estimate_normals(p, U.KNN, 0.0, 30) * ref.normals(p, U.KNN, 0.0, 30)).sum(1)), 1.0,
                           rtol=0, atol=1e-8) or n < 4
    # an integer lattice with max_nn cutting through equal distances: neighbour choice by (d2, index)
    lat = U.lattice(12)
    ln = np.random.default_rng(9).normal(size=lat.shape)
    ln /= np.linalg.norm(ln, axis=1, keepdims=True)
    for search, radius, k in ((U.KNN, 0.0, 5), (U.KNN, 0.0, 20), (U.HYBRID, 1.5, 10)):
        _compare(capi.compute_fpfh_feature(lat, ln, search, radius, k), ref.fpfh(lat, ln, search, radius, k),
                 f"lattice search={search} max_nn={k}")


@pytest.mark.parametrize("search,radius,k", [(U.HYBRID, 0.1, 30), (U.HYBRID, 0.06, 30), (U.KNN, 0.0, 30)])
def test_normals(capi, ref, cloud, search, radius, k):
    import misc3d_amd as m3d
    pts, _ = cloud
    idx, _, m = ref.neighbours(pts, search, radius, k)
    want, gap = U.np_normals(pts, idx, m)
    got, st = capi.estimate_normals(pts, search, radius, k, stats=True)
    ok = gap >= 1e-2
    print(f"normals search={search} radius={radius}: {(~ok).sum()} of {len(pts)} points excluded by the gap")
    assert (~ok).mean() <= 0.01
    cr = np.linalg.norm(np.cross(got[ok], want[ok]), axis=1)
    print(f"  max |n_gpu x n_ref| = {cr.max():.3e}")
    assert cr.max() <= 1e-8
    assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() <= 1e-12
    assert (got[m < 3] == [0.0, 0.0, 1.0]).all()
    assert st["pairs"] == int(m.sum())
    cam = (0.1, -0.2, 0.3)
    o = capi.estimate_normals(pts, search, radius, k, orient_to=cam)
    assert (((np.asarray(cam) - pts) * o).sum(1) >= 0).all()
    assert np.abs(np.linalg.norm(o, axis=1) - 1.0).max() <= 1e-12
    assert np.array_equal(np.abs(o), np.abs(got)) and (np.abs(o[m < 3]) == [0.0, 0.0, 1.0]).all()
    param = ("hybrid", radius, k) if search == U.HYBRID else ("knn", k)
    assert np.array_equal(m3d.features.estimate_normals(pts, param, orient_to=cam), o)


def test_preprocess_fragment_is_the_two_calls(capi, cloud):
    import misc3d_amd as m3d
    pts, nrm = cloud
    pts, nrm = pts[:8000], nrm[:8000]
    voxel = 0.04
    n1 = capi.estimate_normals(pts, U.HYBRID, 2 * voxel, 30, orient_to=(0, 0, 0))
    f1 = capi.compute_fpfh_feature(pts, n1, U.HYBRID, 5 * voxel, 100)
    n2, f2, st = capi.preprocess_fragment(pts, voxel, stats=True)
    assert np.array_equal(n1, n2) and np.array_equal(f1, f2) and st["searches"] == 2
    # normals given: oriented towards the origin, otherwise untouched
    n3, f3 = capi.preprocess_fragment(pts, voxel, normals=nrm)
    assert np.array_equal(n3, U.orient(pts, nrm, (0, 0, 0))) and np.array_equal(np.abs(n3), np.abs(nrm))
    assert np.array_equal(f3, capi.compute_fpfh_feature(pts, n3, U.HYBRID, 5 * voxel, 100))
    pn, pf = m3d.reconstruction.preprocess_fragment(pts, voxel)
    assert np.array_equal(pn, n2) and np.array_equal(pf.T, f2)


def test_end_to_end_registration(capi, ref):
    import misc3d_amd as m3d
    from misc3d_amd import synth
    src, _ = U.three_surface_cloud(6000, seed=21)
    T = synth.rigid_transform(25.0, (1, 2, 3), (0.2, -0.1, 0.3))
    rng = np.random.default_rng(2)
    perm = rng.permutation(len(src))
    dst = np.ascontiguousarray((src @ T[:3, :3].T + T[:3, 3])[perm])
    voxel = 0.04
    g = [m3d.reconstruction.preprocess_fragment(c, voxel) for c in (src, dst)]
    print("points whose SPFH row the host decided:", [capi.preprocess_fragment(c, voxel, stats=True)[2]["tie_points"] for c in (src, dst)])
    r = [ref.preprocess(c, voxel) for c in (src, dst)]
    touched, deferred = [], []
    for k, (gg, rr) in enumerate(zip(g, r)):
        assert np.linalg.norm(np.cross(gg[0], rr[0]), axis=1).max() <= 1e-8 and ((gg[0] * rr[0]).sum(1) > 0).all()
        touched.append(set(_compare(np.ascontiguousarray(gg[1].T), rr[1], f"end to end, cloud {k}", deferred).tolist()))
    # the two correspondence lists are equal except for pairs that touch a point counted under the cap
    g0, g1 = m3d.registration.match_correspondence(g[0][1], g[1][1])
    r0, r1 = m3d.registration.match_correspondence(r[0][1].T, r[1][1].T)
    sg = set(zip((int(v) for v in g0), (int(v) for v in g1)))
    sr = set(zip((int(v) for v in r0), (int(v) for v in r1)))
    for a, b in sg ^ sr:
        assert a in touched[0] or b in touched[1], (a, b)
    print(f"end to end: {len(sg)} correspondences, {len(sg ^ sr)} differ")
    assert len(sg) > 100
    ok, pose, info = m3d.reconstruction.global_registration(src, dst, g[0][1], g[1][1], voxel, seed=3)
    assert ok
    moved = src @ pose[:3, :3].T + pose[:3, 3]
    assert np.sqrt(((moved[perm] - dst) ** 2).sum(1)).mean() < 2 * voxel
    frags = [src, dst, src]
    a = m3d.reconstruction.register_fragment_pairs(frags, None, [(0, 1), (0, 2)], voxel, seeds=[5, 6])
    feats = [m3d.reconstruction.preprocess_fragment(f, voxel)[1] for f in frags]
    b = m3d.reconstruction.register_fragment_pairs(frags, feats, [(0, 1), (0, 2)], voxel, seeds=[5, 6])
    assert len(a) == len(b) == 2
    for x, y in zip(a, b):
        assert x[:3] == y[:3] and np.array_equal(x[3], y[3]) and np.array_equal(x[4], y[4])
    for what, nbad, n in deferred:     # the FPFH cap on both clouds
        assert nbad <= CAP * n, (what, nbad)


def test_four_threads(capi, cloud):
    import misc3d_amd as m3d
    pts, nrm = cloud
    pts, nrm = pts[:10000], nrm[:10000]
    want = m3d.features.compute_fpfh_feature((pts, nrm), ("hybrid", 0.1, 100))
    res = [None] * 4

    def work(i):
        res[i] = m3d.features.compute_fpfh_feature((pts, nrm), ("hybrid", 0.1, 100))

    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for r in res:
        assert r is not None and np.array_equal(r, want)
