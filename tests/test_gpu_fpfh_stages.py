"""The FPFH chain on the device held to the restatement stage by stage (m3d_bench_fpfh_stages, include/misc3d_amd_bench.h), with
no cap and, where the stage is a fixed sequence of IEEE operations, no tolerance.

  A  lists     list_idx / list_d2 / cnt == Ref.neighbours, d2 as bytes
  B  SPFH      the u8 pair counts == fpfh_stage_util.ref_counts on EVERY point (tests/test_fpfh.py shows that no pair of these
               inputs lies within 1e-9 of a bin edge; tie points included: their rows come from the host's libm, which is the
               restatement's), the increment == 100 / (m - 1) as bytes
  C  ties      inner band (32 eps) <= the points the device listed <= outer band (128 eps); the library's band is 64 eps and the
               device's acos may be a few ulp off numpy's on either side
  D  gather    feature_out == assemble(the device's own lists, counts, increments) as BYTES: given its inputs fpfh_fpfh_k is a
               fixed sequence of IEEE operations.  (The whole call is not: the device forms an SPFH entry as count x incr where
               the restatement adds incr count times, roundings of order 1e-14.)
  whole call   feature_out against Ref.fpfh within rtol = atol = 1e-9 on every point
  normals      estimate_normals == Ref.normals as bytes: fpfh_ref.c restates the raw sums and the cyclic Jacobi operation for
               operation, + - * / sqrt only, contraction off on both sides

A library built for another floating-point association (capi.FP_ORDER != 0) is not bit for bit with the restatement: A and the
normals are skipped there, B, C, D and the whole call stay."""
import numpy as np
import pytest

import fpfh_ref_util as U
import fpfh_stage_util as S

pytestmark = pytest.mark.gpu

SEAM = tuple(S.seam_cases())
BIG = ("big_2_0.1_100", "big_2_0.05_30", "big_0_0.0_30", "big_0_0.0_128")
TIE = ("tie6000", "tie6000_moved", "tie1500")
ALL = SEAM + BIG + TIE
CAM = (0.1, -0.2, 0.3)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp("fpfh_ref"))


def _case(ref, name):
    if name in TIE:
        return S.tie_cases(ref)[name]
    return S.big_cases()[name] if name in BIG else S.seam_cases()[name]


_STAGES = {}


def _stages(capi, ref, name):
    """(case, the device's stages, the reference), one device call per case and module"""
    c = _case(ref, name)
    if name not in _STAGES:
        _STAGES[name] = capi.fpfh_stages(c["pts"], c["nrm"], c["search"], c["radius"], c["k"])
    return c, _STAGES[name], S.reference(ref, c)


def _below(cnt, k):
    return np.arange(k)[None, :] < cnt.astype(np.int64)[:, None]


def _exact_only(capi):
    if capi.FP_ORDER != 0:
        pytest.skip("bit for bit with the restatement only in the default association")


@pytest.mark.parametrize("name", ALL)
def test_stage_a_lists(capi, ref, name):
    _exact_only(capi)
    c, g, r = _stages(capi, ref, name)
    finite = np.isfinite(c["pts"]).all(1)
    assert np.array_equal(g["cnt"].astype(np.int64), r["m"])
    assert not g["cnt"][~finite].any()
    live = _below(g["cnt"], c["k"])
    assert np.array_equal(g["list_idx"][live].astype(np.int64), r["idx"][live])
    assert g["list_d2"][live].tobytes() == r["d2"][live].tobytes()
    assert finite[g["list_idx"][live]].all()
    assert (g["list_idx"][~live] == 0xFFFFFFFF).all() and np.isposinf(g["list_d2"][~live]).all()
    assert g["stats"]["pairs"] == int(g["cnt"].sum()) and g["stats"]["searches"] == 1


def _count_failure(capi, c, g, r, i):
    """names the first pair of point i whose bins differ between the library's host evaluator and the restatement"""
    sel = np.nonzero(r["own"] == i)[0]
    pairs = S._pairs12(c["pts"], c["nrm"], r["own"][sel], r["j"][sel])
    lb, lf = capi.fpfh_pair_bins(pairs, features=True)
    bad = np.nonzero((lb != r["bins"][sel]).any(1))[0]
    msg = (f"point {i}, m = {int(r['m'][i])}: device counts {g['spfh_count'][i].tolist()} against {r['counts'][i].tolist()}")
    for t in bad[:3]:
        msg += (f"\n  pair ({i}, {int(r['j'][sel][t])}) at k = {int(r['k'][sel][t])}: library bins {lb[t].tolist()} features "
                f"{lf[t].tolist()}; restatement bins {r['bins'][sel][t].tolist()} features {r['feat'][sel][t].tolist()}")
    if not len(bad):
        msg += "\n  the host evaluator agrees with the restatement on every pair of the point: the device's counting differs"
    return msg


@pytest.mark.parametrize("name", ALL)
def test_stage_b_spfh_integers(capi, ref, name):
    c, g, r = _stages(capi, ref, name)
    assert g["spfh_incr"].tobytes() == S.incr_of(g["cnt"]).tobytes()
    differ = np.nonzero((g["spfh_count"].astype(np.int64) != r["counts"]).any(1))[0]
    may = np.zeros(len(c["pts"]), bool)
    may[r["own"][r["undecided"]]] = True          # (none on these inputs: tests/test_fpfh.py)
    wrong = differ[~may[differ]]
    assert len(wrong) == 0, f"{len(wrong)} points differ; " + _count_failure(capi, c, g, r, int(wrong[0]))
    assert np.array_equal(g["spfh_count"].sum(1, dtype=np.int64), 3 * np.maximum(r["m"] - 1, 0))


@pytest.mark.parametrize("name", ALL)
def test_stage_c_ties(capi, ref, name):
    c, g, r = _stages(capi, ref, name)
    tp = g["tie_points"].astype(np.int64)
    assert g["n_ties"] == len(tp) == g["stats"]["tie_points"]
    assert (np.diff(tp) > 0).all() and (len(tp) == 0 or tp[-1] < len(c["pts"]))
    listed = np.zeros(len(c["pts"]), bool)
    listed[tp] = True
    inner, _, outer = r["bands"]
    print(f"{name}: {len(tp)} points listed; {int(inner.sum())} / {int(outer.sum())} in the 32 / 128 eps bands")
    if capi.FP_ORDER == 0:
        assert not (inner & ~listed).any(), np.nonzero(inner & ~listed)[0][:5]
        assert not (listed & ~outer).any(), np.nonzero(listed & ~outer)[0][:5]
    if not c.get("estimated"):
        assert len(tp) == 0                    # given, well-separated normals list nobody
    if name == "tie6000":
        assert g["n_ties"] > 64                # more than one block of fpfh_tie_scatter_k
    if name == "tie1500":
        assert g["n_ties"] > 0 and c["k"] > 64     # fpfh_tie_gather_k strides its list twice


@pytest.mark.parametrize("name", ALL)
def test_stage_d_gather_bit_for_bit(capi, ref, name):
    c, g, _ = _stages(capi, ref, name)
    want = S.assemble(g["list_idx"], g["list_d2"], g["cnt"], g["spfh_count"], g["spfh_incr"])
    same = (g["feature"].view(np.uint64) == want.view(np.uint64)).all(1)
    assert same.all(), (int((~same).sum()), int(np.nonzero(~same)[0][0]), np.abs(g["feature"] - want).max())
    assert g["feature"].tobytes() == want.tobytes()
    call, st = capi.compute_fpfh_feature(c["pts"], c["nrm"], c["search"], c["radius"], c["k"], stats=True)
    assert call.tobytes() == g["feature"].tobytes()
    assert {k: v for k, v in st.items() if not k.startswith("ms_")} == {k: v for k, v in g["stats"].items() if not k.startswith("ms_")}


@pytest.mark.parametrize("name", ALL)
def test_whole_call(capi, ref, name):
    c, g, _ = _stages(capi, ref, name)
    want = ref.fpfh(c["pts"], c["nrm"], c["search"], c["radius"], c["k"])
    bad = U.differing_points(g["feature"], want)
    assert len(bad) == 0, (len(bad), int(bad[0]), np.abs(g["feature"] - want).max())
    assert U.group_sums_ok(g["feature"]).all()


def test_every_seam_is_hit(capi, ref):
    """the clouds sit on the seams they were built for, by the device's own counts, and what each seam promises holds"""
    seen = set()
    for name in SEAM:
        c, g, _ = _stages(capi, ref, name)
        cnt = g["cnt"].astype(np.int64)
        finite = np.isfinite(c["pts"]).all(1)
        if "m_all" in c:
            assert (cnt[finite] == c["m_all"]).all(), name
        if "m_each" in c:
            assert np.array_equal(cnt, c["m_each"]), name
        if name.startswith("m"):
            seen |= set(cnt.tolist())
        if "m_max" in c:
            assert cnt.max() == c["m_max"], name
        assert not g["feature"][cnt <= 1].any() and not g["spfh_count"][cnt <= 1].any(), name
        if "base" in c:
            _, b, _ = _stages(capi, ref, c["base"])
            keep = c["keep"]
            assert len(keep) == len(c["pts"]) - 7 and not finite[np.setdiff1d(np.arange(len(finite)), keep)].any()
            assert not g["feature"][~finite].any() and not g["spfh_count"][~finite].any() and not g["spfh_incr"][~finite].any()
            assert g["feature"][keep].tobytes() == b["feature"].tobytes(), name
            assert np.array_equal(g["cnt"][keep], b["cnt"]) and np.array_equal(g["spfh_count"][keep], b["spfh_count"])
            live = _below(b["cnt"], c["k"])
            assert np.array_equal(keep[b["list_idx"][live]], g["list_idx"][keep][live])       # sidx is no identity here
    assert seen >= set(S.M_VALUES), sorted(seen)
    # the Hybrid cut at equality: strict <
    for name, inside in (("lattice_r2_out", False), ("lattice_r2_in", True)):
        c, g, _ = _stages(capi, ref, name)
        d2 = g["list_d2"][_below(g["cnt"], c["k"])]
        assert (d2 == 4.0).any() == inside and d2.max() == (4.0 if inside else 3.0)
    # the u8 count's ceiling
    c, g, _ = _stages(capi, ref, "flat_knn128")
    want = np.zeros(33, np.int64)
    want[[5, 16, 27]] = 127
    assert (g["spfh_count"] == want).all()
    assert np.allclose(g["feature"], want / 127 * 200.0, rtol=0, atol=1e-9)
    # duplicates: entry 0 of a later copy is the first copy, the copies come with d2 == 0
    c, g, _ = _stages(capi, ref, "duplicates")
    for group in c["copies"]:
        for i in group:
            assert g["list_idx"][i, :len(group)].tolist() == list(group) and not g["list_d2"][i, :len(group)].any()
    c, g, _ = _stages(capi, ref, "one_point_70")
    assert not g["list_d2"][:, :70].any()
    assert g["feature"].tobytes() == (g["spfh_count"].astype(np.float64) * g["spfh_incr"][:, None]).tobytes()     # out = own


def _normals_equal(got, want, what):
    same = (got.view(np.uint64) == want.view(np.uint64)).all(1)
    if not same.all():
        i = int(np.nonzero(~same)[0][0])
        dev = np.abs(got - want).max()
        raise AssertionError(f"{what}: {int((~same).sum())} of {len(same)} normals differ, largest deviation {dev:.3e}; first at "
                             f"{i}: {got[i].tolist()} against {want[i].tolist()}")


@pytest.mark.parametrize("name", SEAM)
def test_normals_bit_for_bit_on_seams(capi, ref, name):
    _exact_only(capi)
    c = _case(ref, name)
    a = (c["search"], c["radius"], c["k"])
    plain = capi.estimate_normals(c["pts"], *a)
    _normals_equal(plain, ref.normals(c["pts"], *a), name)
    _normals_equal(capi.estimate_normals(c["pts"], *a, orient_to=CAM), ref.normals(c["pts"], *a, orient_to=CAM), name + " oriented")
    _, _, m = ref.neighbours(c["pts"], *a)
    assert (plain[m < 3] == [0.0, 0.0, 1.0]).all()
    if "base" in c:
        assert plain[c["keep"]].tobytes() == capi.estimate_normals(_case(ref, c["base"])["pts"], *a).tobytes()


@pytest.mark.parametrize("search,radius,k", [(U.HYBRID, 0.1, 30), (U.HYBRID, 0.06, 30), (U.KNN, 0.0, 30)])
def test_normals_bit_for_bit(capi, ref, search, radius, k):
    _exact_only(capi)
    pts = S.big_cases()[BIG[0]]["pts"]
    _normals_equal(capi.estimate_normals(pts, search, radius, k), ref.normals(pts, search, radius, k), "plain")
    _normals_equal(capi.estimate_normals(pts, search, radius, k, orient_to=CAM), ref.normals(pts, search, radius, k, orient_to=CAM),
                   "oriented")


def test_preprocess_fragment_normals_bit_for_bit(capi, ref):
    """lists of 30 on the grid class of 100; the descriptors on top of them within 1e-9 on every point"""
    c = S.tie_cases(ref)["tie6000"]
    voxel = 0.04
    nrm, feat, st = capi.preprocess_fragment(c["pts"], voxel, stats=True)
    if capi.FP_ORDER == 0:
        _normals_equal(nrm, c["nrm"], "preprocess_fragment")
        assert st["tie_points"] == _stages(capi, ref, "tie6000")[1]["n_ties"]
    want = ref.fpfh(c["pts"], nrm, U.HYBRID, 5 * voxel, 100)
    assert len(U.differing_points(feat, want)) == 0 and st["searches"] == 2
