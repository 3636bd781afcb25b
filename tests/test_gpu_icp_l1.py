"""m3d_registration_icp_plane_l1 on the MI355X against the restatement of its contract (tests/icp_l1_ref_util.py, exact sums):
iteration counts, correspondence arrays and fitness equal, inlier_rmse to rel 1e-9, poses to atol 1e-9 -- the bar of the plane
call (rule 8) -- on the plane call's cases, at the workgroup seams of the iteration kernel, and where a residual is exactly
zero; run-to-run bit equality; the Python API.  tests/test_icp_l1.py guards every input used here: the order of the sums
decides nothing on it."""
import numpy as np
import pytest

import icp_l1_ref_util as lu
import icp_ref_util as iu
from voxel_ref_util import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return iu.IcpRef(tmp_path_factory.mktemp("icp_ref"))


@pytest.fixture(scope="module")
def dev(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device")
    return capi


def _run(dev, c, l1=True):
    return dev.registration_icp_plane(c["src"], c["dst"], c["dst_normals"], c["max_dist"], c["init"], c["max_iteration"],
                                      want_correspondences=True, l1=l1)


def _check(got, exp):
    T, st, corr = got
    print("iterations", st["iterations"], exp["iterations"], "fitness", st["fitness"], exp["fitness"], "rmse", st["inlier_rmse"],
          exp["inlier_rmse"], "pose diff", np.abs(T - exp["T"]).max())
    assert st["iterations"] == exp["iterations"] and st["converged"] == exp["converged"]
    assert np.array_equal(corr, exp["corr"])
    assert st["fitness"] == exp["fitness"] and st["correspondences"] == exp["correspondences"]
    assert st["inlier_rmse"] == pytest.approx(exp["inlier_rmse"], rel=1e-9, abs=0)
    assert np.allclose(T, exp["T"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("name", lu.CASES)
def test_matches_the_restatement(dev, ref, name):
    c, exp = lu.expected(ref, name)
    got = _run(dev, c)
    _check(got, exp)
    T, st, corr = got
    if name in ("nonfinite", "zero_residual"):
        # a NaN normal / an infinite weight in the record: the identity update, the initial pose bit for bit
        assert st["iterations"] == 1 and np.array_equal(bits(T), bits(np.eye(4) if c["init"] is None else c["init"]))
    if name == "zero_residual":
        assert corr[7] == 123
    if name == "nonfinite":
        assert c["nan_normal_at"] in corr
    if name == "duplicates":
        assert np.all(corr < len(c["dst"]) - 300)


@pytest.mark.parametrize("n", lu.SEAM_SIZES)
def test_iteration_kernel_workgroup_seams(dev, ref, n):
    """the workgroup edge (255, 256, 257 moving points) and 65 workgroup records (the 64-stride edge of the final launch)"""
    c, exp = lu.expected(ref, n)
    assert c["max_iteration"] <= 3 and len(c["src"]) == n
    _check(_run(dev, c), exp)


def test_a_long_run_ends_at_the_true_pose(dev):
    """thirty iterations allowed: too many to compare roundings (icp_l1_ref_util.case), held to the pose the pair was made with"""
    c = lu.long_case()
    T, st, corr = _run(dev, c)
    print("iterations", st["iterations"], "converged", st["converged"], "pose error", np.abs(T - c["T"]).max())
    assert st["iterations"] > lu.MAX_ITERATION and st["fitness"] == 1.0 and np.all(corr >= 0)
    assert np.allclose(T, c["T"], rtol=0, atol=1e-3)


def test_the_weights_change_the_estimate_and_only_the_estimate(dev):
    """one iteration of both plane estimators from the same pose: the same first correspondence search, another update"""
    c = dict(iu.case("small"), max_iteration=1)
    T1, st1, _ = _run(dev, c, l1=True)
    T2, st2, _ = _run(dev, c, l1=False)
    assert st1["iterations"] == st2["iterations"] == 1
    assert not np.array_equal(T1, T2) and np.allclose(T1, T2, rtol=0, atol=5e-3)
    for T in (T1, T2):
        assert np.abs(T - c["T"]).max() < np.abs(c["init"] - c["T"]).max()


def test_deterministic(dev):
    c = iu.case("duplicates")
    a, b = _run(dev, c), _run(dev, c)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[2], b[2]) and a[1]["inlier_rmse"] == b[1]["inlier_rmse"]


def test_python_api(dev):
    import misc3d_amd as m3d
    c = iu.case("small")
    Tp, st = m3d.registration_icp(c["src"], (c["dst"], c["dst_normals"]), c["max_dist"], c["init"], estimation="point_to_plane_l1")
    Tc, stc = dev.registration_icp_plane(c["src"], c["dst"], c["dst_normals"], c["max_dist"], c["init"], l1=True)
    assert np.array_equal(bits(Tp), bits(Tc)) and st["iterations"] == stc["iterations"]
    Tl2, _ = m3d.registration_icp(c["src"], (c["dst"], c["dst_normals"]), c["max_dist"], c["init"], estimation="point_to_plane")
    assert not np.array_equal(Tp, Tl2)
