"""Every radius-grid search at every rung of the cell-table ladder (radius_grid_geom, m3d_grid_geom.hpp) on the MI355X.

The kernels behind the registration validation, the ICP family, boundary detection, ProximityExtractor, radius_neighbors and
orient_normals_mst take the grid's K and cell edge on trust; the scenes of tests/grid_ladder_util.py (a few islands of points
spread over 10 to 1e10 radii) put each of them on the rungs its K0 can reach -- K kept, K halved, the cell doubled once to 25
times, the branch for more than 1e9 cells per axis, a table seven cells thick -- and every case first asserts through the hook
m3d_bench_radius_grid_geom that it sits on the rung it is meant for.  Each consumer is held to the reference its own tests use,
with their comparisons: no tolerance here is new.  tests/test_grid_ladder.py shows on the CPU that the references alone make the
cases non-vacuous (neighbours between 2/3 r and r away, ties met, other islands left alone).

The K0 = 3 cases at extent / r = 170 and 300 sit where the ladder used to halve K without recomputing the cell (K h = 0.667 r): the
validation then missed neighbours in the corners of its 3 x 3 x 3 block and counted low."""
import math
from fractions import Fraction

import numpy as np
import pytest

import boundary_ref_util as bru
import grid_ladder_util as gl
import icp_ref_util as iu
import ppf_train_ref_util as tu
import reg_sums_ref_util as ru
from proximity_ref_util import build_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device")
    return capi


@pytest.fixture(scope="module")
def prox_ref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("prox_ref"))


@pytest.fixture(scope="module")
def icp_ref(tmp_path_factory):
    return iu.IcpRef(tmp_path_factory.mktemp("icp_ref"))


@pytest.fixture(scope="module")
def train_ref(tmp_path_factory):
    return tu.TrainRef(tmp_path_factory.mktemp("ppf_train_ref"))


def _on_rung(capi, pts, edge, k0, want):
    """the library's own geometry puts the cloud on the rung the case is about (K, doublings of the cell) -> the cell edge"""
    K, doublings, h = gl.rung(pts, edge, k0, hook=capi.radius_grid_geom)
    assert (K, doublings) == want, ("the scene left its rung", K, doublings, want)
    assert K * h >= 1.0009 * edge
    return h


# ---------------------------------------------------------------------------------------------- registration validation
def _records(capi, p, **cfg):
    old = capi.set_config(**cfg)
    try:
        counts, sums = [], []
        with capi.RegSession(p["src"], p["dst"], p["cs"], p["cd"], threshold=p["thr"], **p["kw"]) as sess:
            while (m := sess.begin_chunk()) is not None:
                c, s = sess.validate(0, m)
                counts.append(c.copy())
                sums.append(s.copy())
                sess.replay(c, s)
            T, st = sess.finish()
    finally:
        capi.restore_config(old)
    return np.concatenate(counts), np.concatenate(sums), T, st


@pytest.mark.parametrize("case", gl.REG_CASES, ids=[c["id"] for c in gl.REG_CASES])
def test_registration_validation(dev, orc, case):
    """registration_ransac and the RegSession records against oracle.registration_ransac (exhaustive search): best_index,
    validations and fitness equal, the pose bit-equal; every chunk's counts equal and sums within rtol 1e-12 across the candidate
    cache off / forced, the fp32 screen off / on (pruning off: a pruned hypothesis reports a partial sum), and the call's results
    equal with pruning on as well -- as test_registration_candidate_cache_is_exact compares them."""
    p = gl.reg_problem(**case["problem"])
    k_cfg = case["k_cfg"]
    assert dev.reg_grid_k0(k_cfg, len(p["dst"])) == case["k0"]
    _on_rung(dev, p["dst"], p["thr"], case["k0"], case["rung"])
    o = gl.reg_reference(orc, case)
    assert o.best_index >= 0 and o.fitness > 0.3
    res = {}
    for prune in (0, 1):
        for cache in (0, 2):
            for screen in (0, 1):
                res[prune, cache, screen] = _records(dev, p, reg_cells_per_radius=k_cfg, reg_prune=prune, reg_cache=cache,
                                                     reg_fp32_screen=screen)
    c0, s0, T0, st0 = res[0, 0, 0]
    print("records", len(c0), "best count", int(c0.max()), "of", len(p["src"]), "oracle fitness", o.fitness, "got", st0["fitness"])
    assert len(c0) >= 10
    assert st0["best_index"] == o.best_index and st0["validations"] == o.validations and st0["fitness"] == o.fitness
    assert np.array_equal(T0.view(np.uint64), o.T.view(np.uint64))
    for (prune, cache, screen), (c, s, T, st) in res.items():
        if prune == 0:
            assert np.array_equal(c, c0) and np.allclose(s, s0, rtol=1e-12, atol=0.0), (cache, screen)
        assert np.array_equal(T, T0), (prune, cache, screen)
        for k in ("best_index", "iterations", "validations", "est_k", "fitness", "inlier_rmse"):
            assert st[k] == st0[k], (prune, cache, screen, k)
    old = dev.set_config(reg_cells_per_radius=k_cfg)
    try:
        T, st = dev.registration_ransac(p["src"], p["dst"], p["cs"], p["cd"], threshold=p["thr"], **p["kw"])
    finally:
        dev.restore_config(old)
    assert st["best_index"] == o.best_index and st["validations"] == o.validations and st["fitness"] == o.fitness
    assert np.array_equal(T.view(np.uint64), o.T.view(np.uint64))
    assert st["inlier_rmse"] == pytest.approx(o.inlier_rmse, rel=1e-12)


# ---------------------------------------------------------------------------------------------- the ICP family (K0 = 4)
def _check_icp(got, exp):                                         # test_gpu_icp.py's _check
    T, st, corr = got
    assert st["iterations"] == exp["iterations"] and st["converged"] == exp["converged"]
    assert np.array_equal(corr, exp["corr"])
    assert st["fitness"] == exp["fitness"] and st["correspondences"] == exp["correspondences"]
    assert st["inlier_rmse"] == pytest.approx(exp["inlier_rmse"], rel=1e-9, abs=0)
    assert np.allclose(T, exp["T"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("ratio,variant", gl.K0_4_RUNGS)
def test_icp_family(dev, orc, icp_ref, ratio, variant):
    """registration_icp and registration_icp_plane against tests/cpp/icp_ref.c, registration_icp against the oracle as well,
    icp_sums against the exhaustive correspondences and the exact sums, information_matrix entry by entry -- the target carries
    exact duplicates at its end (nearest_idx's lowest-index rule under a halved K and a doubled cell) and a non-finite row."""
    c = gl.icp_problem(ratio, variant)
    _on_rung(dev, c["dst"], c["max_dist"], 4, gl.NN_RUNGS[(4, ratio, variant)])
    args = (c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"])
    got = dev.registration_icp(*args, want_correspondences=True)
    _check_icp(got, icp_ref.icp(*args, None))
    T, st, corr = got
    n0 = c["n_finite"]
    assert st["fitness"] > 0.5 and np.all(corr < n0) and np.isin(c["dup_of"], corr).sum() >= 6      # ties met, the lower index won
    oT, ofit, orm, oit, ocorr = orc.registration_icp(*args[:4], max_iter=c["max_iteration"], rel_fitness=1e-6, rel_rmse=1e-6)
    assert st["iterations"] == oit and np.array_equal(corr, ocorr)
    assert st["correspondences"] == int((ocorr >= 0).sum()) and st["fitness"] == ofit
    assert st["inlier_rmse"] == pytest.approx(orm, rel=1e-9, abs=1e-15)
    assert np.allclose(T, oT, rtol=0, atol=1e-9)
    plane = dev.registration_icp_plane(c["src"], c["dst"], c["dst_normals"], c["max_dist"], c["init"], c["max_iteration"],
                                       want_correspondences=True)
    _check_icp(plane, icp_ref.icp(*args, c["dst_normals"]))
    assert np.all(plane[2] < n0)
    # one evaluation of the step under the initial pose: the hook and the information matrix
    ex = ru.IcpExact(c["src"], c["dst"], c["max_dist"], c["init"])
    sums, hcorr = dev.icp_sums(c["src"], c["dst"], c["max_dist"], c["init"])
    assert np.array_equal(hcorr, ex.corr) and sums[1] == ex.count and ex.count > 0.5 * len(c["src"])
    assert not np.isnan(sums).any()
    ratios = ex.ratios(sums)
    print("RATIO", ratio, variant, ratios)
    assert max(ratios.values()) <= 1.0, ratios
    info, count = dev.information_matrix(c["src"], c["dst"], c["max_dist"], c["init"])
    assert count == ex.count and info[3, 3] == info[4, 4] == info[5, 5] == ex.count
    assert ru.same_bits(info, info.T)
    for (a, b), (value, bound) in ru.info_entries(ex.info, ex.count).items():
        assert abs(Fraction(float(info[a, b])) - value) <= bound, (a, b, float(info[a, b]), float(value), float(bound))


# ---------------------------------------------------------------------------------------------- the K0 = 1 consumers
@pytest.mark.parametrize("search,max_nn", [(bru.RADIUS, 0), (bru.HYBRID, 30)], ids=["radius", "hybrid"])
@pytest.mark.parametrize("ratio,variant", gl.SURFACE_RUNGS)
def test_detect_boundary_points(dev, orc, ratio, variant, search, max_nn):
    sc = gl.surface_scene(ratio, variant)
    _on_rung(dev, sc["pts"], sc["r"], 1, gl.surface_rung(ratio, variant))
    ref = bru.reference(sc["pts"], sc["normals"], search, sc["r"], max_nn, 90.0, orc.j3x3_smallest_eigvec)
    got = dev.detect_boundary_points(sc["pts"], sc["normals"], search, sc["r"], max_nn, 90.0).astype(np.int64)
    assert np.array_equal(got, np.unique(got)) and got[-1] < len(sc["pts"])
    assert bru.compare(got, ref) == 0
    assert 0.05 * len(sc["pts"]) < len(got) < 0.9 * len(sc["pts"])        # neither everything nor nothing


EVALUATORS = (dict(kind="distance", dist=0.8), dict(kind="normals", angle=4.0), dict(kind="distance_normals", dist=0.9, angle=-6.0))


@pytest.mark.parametrize("ratio,variant", gl.SURFACE_RUNGS)
def test_proximity_segment(dev, prox_ref, ratio, variant):
    """clusters, their order and the labels equal tests/cpp/proximity_ref.c's for the three evaluators; the reported cell edge
    is the hook's for the same cloud"""
    sc = gl.surface_scene(ratio, variant)
    h = _on_rung(dev, sc["pts"], sc["r"], 1, gl.surface_rung(ratio, variant))
    r = sc["r"]
    for ev in EVALUATORS:
        kw = dict(dist=ev.get("dist", 0.0) * r, angle=ev.get("angle", 0.0), normals=None if ev["kind"] == "distance" else sc["normals"])
        exp = prox_ref.segment(sc["pts"], r, ev["kind"], **kw)
        off, idx, lab, st = dev.proximity_segment(sc["pts"], r, ev["kind"], kw["dist"], kw["angle"], kw["normals"], stats=True)
        got = [idx[off[c]:off[c + 1]].astype(np.int64).tolist() for c in range(len(off) - 1)]
        assert st["cell_edge"] == h
        assert got == exp[0], ev
        assert np.array_equal(lab.astype(np.int64), exp[1]), ev
        assert len(got) >= len(set(sc["island"].tolist()))             # no cluster spans two islands ...
        assert all(len(set(sc["island"][[i for i in cl if i < len(sc["island"])]].tolist())) == 1 for cl in got if len(cl) > 1)
        assert len(got[0]) > 50                                          # ... and the islands are not dust


@pytest.mark.parametrize("ratio,variant", gl.SURFACE_RUNGS)
def test_radius_neighbors(dev, ratio, variant):
    """every row's list equals the exhaustive one in (d2, index) order, d2 bit for bit"""
    sc = gl.surface_scene(ratio, variant)
    pts, r = sc["pts"], sc["r"]
    _on_rung(dev, pts, r, 1, gl.surface_rung(ratio, variant))
    off, idx, d2 = dev.radius_neighbors(pts, r)
    r2 = r * r
    total = 0
    with np.errstate(invalid="ignore"):
        for i in range(len(pts)):
            dx, dy, dz = pts[:, 0] - pts[i, 0], pts[:, 1] - pts[i, 1], pts[:, 2] - pts[i, 2]
            e2 = (dx * dx + dy * dy) + dz * dz
            sel = np.flatnonzero(e2 <= r2)
            sel = sel[sel != i]
            sel = sel[np.lexsort((sel, e2[sel]))]
            lo, hi = int(off[i]), int(off[i + 1])
            assert np.array_equal(idx[lo:hi].astype(np.int64), sel), i
            assert np.array_equal(d2[lo:hi].view(np.uint64), e2[sel].view(np.uint64)), i
            total += len(sel)
    assert int(off[-1]) == total == len(idx) and total > 8 * len(pts)


@pytest.mark.parametrize("ratio,variant", gl.SURFACE_RUNGS)
def test_orient_normals_mst(dev, train_ref, ratio, variant):
    """parent, normals and stats equal the heap walk's byte for byte; only the seed's island is touched"""
    c = gl.orient_problem(ratio, variant)
    _on_rung(dev, c["points"], c["radius"], 1, gl.surface_rung(ratio, variant))
    args = dict(points=c["points"], normals=c["normals"], radius=c["radius"], seed=c["seed"])
    gn, gp, gs = dev.orient_normals_mst(**args)
    wn, wp, ws = train_ref.orient(**args)
    assert np.array_equal(gp, wp)
    assert gn.tobytes() == wn.tobytes()
    assert {k: gs[k] for k in tu.STATS} == ws
    assert 1 <= gs["rounds"] <= math.ceil(math.log2(len(gp))) + 1
    other = c["island"] != c["island"][c["seed"]]
    assert (gp[other] == -2).all() and gn[other].tobytes() == c["normals"][other].tobytes()
    assert gs["component"] > 0.9 * (~other).sum() and gs["flips"] > 0.2 * gs["component"]
