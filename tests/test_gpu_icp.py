"""m3d_registration_icp_plane and m3d_multi_scale_icp on the MI355X against the plain-C restatement of the contract
(tests/cpp/icp_ref.c, levels from tests/cpp/voxel_ref.c): iteration counts, correspondence arrays and fitness equal,
inlier_rmse to rel 1e-9, poses to atol 1e-9 (the project's n-point bar) -- point-to-point through the same
reference file; run-to-run and thread-to-thread bit equality; the multi-scale call against the reference and, bit for bit,
against the same levels composed from the public calls; the Python API and the C++ mirror; the plane kernel at the
workgroup seams, against the numpy restatement.  tests/test_icp.py guards every input used here (the seam test its own): the
order of the reference's sums decides nothing on it."""
import os
import subprocess
import threading

import numpy as np
import pytest

import icp_ref_util as iu
from voxel_ref_util import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return iu.IcpRef(tmp_path_factory.mktemp("icp_ref"))


@pytest.fixture(scope="module")
def dev(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device")
    return capi


@pytest.fixture(scope="module")
def multi():
    return iu.multi_case()


def _run(dev, c, plane):
    if plane:
        return dev.registration_icp_plane(c["src"], c["dst"], c["dst_normals"], c["max_dist"], c["init"], c["max_iteration"],
                                          want_correspondences=True)
    return dev.registration_icp(c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"], want_correspondences=True)


def _check(got, exp):
    T, st, corr = got
    print("iterations", st["iterations"], exp["iterations"], "fitness", st["fitness"], exp["fitness"], "rmse", st["inlier_rmse"],
          exp["inlier_rmse"], "pose diff", np.abs(T - exp["T"]).max())
    assert st["iterations"] == exp["iterations"] and st["converged"] == exp["converged"]
    assert np.array_equal(corr, exp["corr"])
    assert st["fitness"] == exp["fitness"] and st["correspondences"] == exp["correspondences"]
    assert st["inlier_rmse"] == pytest.approx(exp["inlier_rmse"], rel=1e-9, abs=0)
    assert np.allclose(T, exp["T"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("name", iu.CASES)
def test_point_to_plane_matches_the_reference(dev, ref, name):
    c = iu.case(name)
    exp = ref.icp(c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"], c["dst_normals"])
    got = _run(dev, c, True)
    _check(got, exp)
    T, st, corr = got
    if name == "refine":
        assert st["converged"] == 1 and np.allclose(T, c["T"], rtol=0, atol=1e-3)
    if name == "no_convergence":
        assert st["converged"] == 0 and st["iterations"] == 2
    if name == "duplicates":
        assert np.all(corr < len(c["dst"]) - 300)
    if name == "identity_init":
        assert st["iterations"] >= 2
    if name == "nonfinite":
        assert st["iterations"] == 1 and np.array_equal(bits(T), bits(c["init"])) and c["nan_normal_at"] in corr
    if name == "no_correspondences":
        assert st["fitness"] == 0.0 and np.array_equal(bits(T), bits(c["init"])) and np.all(corr == -1)


@pytest.mark.parametrize("name", iu.CASES)
def test_point_to_point_matches_the_same_reference(dev, ref, name):
    c = iu.case(name)
    _check(_run(dev, c, False), ref.icp(c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"], None))


@pytest.mark.parametrize("n", [255, 256, 257, 16385])
def test_plane_iteration_kernel_workgroup_seams(dev, ref, n):
    """the workgroup edge (255, 256, 257 moving points) and 65 workgroup records (the 64-stride edge of the final launch) of
    the frame the plane kernel shares with the coloured one (tests/test_gpu_colored_icp.py runs the same sizes), against the
    numpy restatement; the input is guarded here: the plain-C restatement agrees with it and, summed in descending order, with
    itself"""
    c = iu.sized_case(n)
    assert c["max_iteration"] <= 3 and len(c["src"]) == n
    args = (c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"], c["dst_normals"])
    with np.errstate(invalid="ignore"):
        exp = iu.icp_numpy(*args)
    up, down = ref.icp(*args, order=1), ref.icp(*args, order=-1)
    for r in (up, down):
        assert r["iterations"] == exp["iterations"] and np.array_equal(r["corr"], exp["corr"])
    assert exp["correspondences"] > 0.9 * n
    _check(_run(dev, c, True), exp)


def test_deterministic_alone_and_from_two_threads(dev):
    cases = [iu.case("refine"), iu.case("duplicates")]
    alone = [_run(dev, c, True) for c in cases]
    for c, a in zip(cases, alone):
        again = _run(dev, c, True)
        assert np.array_equal(bits(again[0]), bits(a[0])) and np.array_equal(again[2], a[2])
        assert again[1]["inlier_rmse"] == a[1]["inlier_rmse"]
    out = [None, None]

    def work(k):
        out[k] = [_run(dev, cases[k], True) for _ in range(3)]
    ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for k in range(2):
        assert out[k] is not None
        for r in out[k]:
            assert np.array_equal(bits(r[0]), bits(alone[k][0])) and np.array_equal(r[2], alone[k][2])
            assert r[1]["inlier_rmse"] == alone[k][1]["inlier_rmse"] and r[1]["iterations"] == alone[k][1]["iterations"]


@pytest.mark.parametrize("three", [True, False])
@pytest.mark.parametrize("plane", [True, False])
def test_multi_scale_matches_the_reference(dev, ref, multi, three, plane):
    m = multi
    vs, its = iu.levels_of(m["voxel"], three)
    nrm = m["dst_normals"] if plane else None
    exp = ref.multi_scale(m["src"], m["dst"], vs, its, m["max_dist"], m["init"], nrm)
    T, info, levels = dev.multi_scale_icp(m["src"], m["dst"], vs, its, m["max_dist"], m["init"], int(plane), nrm)
    print([(l["n_src"], l["n_dst"], l["icp"]["iterations"], round(l["ms_down_sample"], 3), round(l["ms_icp"], 3),
            round(l["ms_information"], 3)) for l in levels], "pose diff", np.abs(T - exp["T"]).max())
    assert len(levels) == len(vs)
    for got, e in zip(levels, exp["levels"]):
        assert (got["n_src"], got["n_dst"]) == (e["n_src"], e["n_dst"])
        assert got["icp"]["iterations"] == e["iterations"] and got["icp"]["fitness"] == e["fitness"]
    assert np.allclose(T, exp["T"], rtol=0, atol=1e-9)
    assert info[5, 5] == exp["n_info"] == exp["info"][5, 5]
    assert np.abs(info - exp["info"]).max() <= 1e-9 * np.abs(exp["info"]).max()


@pytest.mark.parametrize("plane", [True, False])
def test_multi_scale_equals_the_public_calls_composed(dev, multi, plane):
    m = multi
    vs, its = iu.levels_of(m["voxel"], True)
    nrm = m["dst_normals"] if plane else None
    T, info, levels = dev.multi_scale_icp(m["src"], m["dst"], vs, its, m["max_dist"], m["init"], int(plane), nrm)
    ls = dev.voxel_down_sample_multi(m["src"], vs)
    ld = dev.voxel_down_sample_multi(m["dst"], vs, nrm)
    cur = m["init"]
    for l, (s, d, it) in enumerate(zip(ls, ld, its)):
        if plane:
            cur, st = dev.registration_icp_plane(s["points"], d["points"], d["normals"], m["max_dist"], cur, it)
        else:
            cur, st = dev.registration_icp(s["points"], d["points"], m["max_dist"], cur, it)
        for k in ("fitness", "inlier_rmse", "correspondences", "iterations", "converged"):
            assert levels[l]["icp"][k] == st[k], (l, k)
        assert (levels[l]["n_src"], levels[l]["n_dst"]) == (len(s["points"]), len(d["points"]))
    assert np.array_equal(bits(T), bits(cur))
    info2, cnt = dev.information_matrix(m["src"], m["dst"], vs[-1] * 1.4, cur)
    assert np.array_equal(bits(info), bits(info2)) and info[5, 5] == cnt


def test_python_api(dev, multi):
    import misc3d_amd as m3d
    m = multi
    rec = m3d.reconstruction

    class Target:
        points, normals = m["dst"], m["dst_normals"]
    T, info = rec.refine_fragment_pair(m["src"], Target(), iu.MULTI_VOXEL, m["init"])
    v32 = np.float32(iu.MULTI_VOXEL)
    sizes = [float(v32), float(v32 / np.float32(2)), float(v32 / np.float32(4))]
    assert sizes[0] != iu.MULTI_VOXEL        # (single-precision levels: what the reference's `const float` forms)
    T2, info2 = rec.multi_scale_icp(m["src"], (m["dst"], m["dst_normals"]), sizes, [50, 30, 15], float(v32) * 1.4, m["init"],
                                    rec.LocalRefineMethod.Point2PlaneICP)
    assert np.array_equal(bits(T), bits(T2)) and np.array_equal(bits(info), bits(info2))
    assert np.allclose(T, m["T"], rtol=0, atol=1e-3)
    To, info_o, lv = rec.fragment_odometry(m["src"], Target(), iu.MULTI_VOXEL, m["init"], "point_to_point", stats=True)
    To2, _, _ = dev.multi_scale_icp(m["src"], m["dst"], [float(v32)], [50], float(v32) * 1.4, m["init"], 0)
    assert np.array_equal(bits(To), bits(To2)) and len(lv) == 1 and lv[0]["icp"]["iterations"] >= 3
    c = iu.case("small")
    Tp, st = m3d.registration_icp(c["src"], (c["dst"], c["dst_normals"]), c["max_dist"], c["init"], estimation="point_to_plane")
    Tc, stc = dev.registration_icp_plane(c["src"], c["dst"], c["dst_normals"], c["max_dist"], c["init"])
    assert np.array_equal(bits(Tp), bits(Tc)) and st["iterations"] == stc["iterations"]
    Td, _ = m3d.registration_icp(c["src"], c["dst"], c["max_dist"], c["init"])          # the default is unchanged
    assert np.array_equal(bits(Td), bits(dev.registration_icp(c["src"], c["dst"], c["max_dist"], c["init"])[0]))


def test_cpp_mirror(dev, tmp_path):
    exe = str(tmp_path / "icp_mirror")
    lib = os.path.join(ROOT, "misc3d_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_icp_mirror.cpp"), "-o", exe, "-L", lib, "-lmisc3d_amd", "-lpthread",
                    "-Wl,-rpath," + lib], check=True)
    p = iu.icp_pair(6001, seed=31)
    v = 0.05
    init = iu.offset_pose(p["T"], 1.0, (0.01, -0.005, 0.008))
    blob = tmp_path / "pair.bin"
    blob.write_bytes(np.array([len(p["src"]), len(p["dst"])], dtype=np.uint64).tobytes() + p["src"].tobytes() + p["dst"].tobytes()
                     + p["dst_normals"].tobytes() + np.ascontiguousarray(init).tobytes() + np.float64(v).tobytes())
    r = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")

    def words(line):
        return np.array([int(t, 16) for t in line.split()], dtype=np.uint64)
    v32 = np.float32(v)
    sizes = [float(v32), float(v32 / np.float32(2)), float(v32 / np.float32(4))]
    T, info, _ = dev.multi_scale_icp(p["src"], p["dst"], sizes, [50, 30, 15], float(v32) * 1.4, init, 1, p["dst_normals"])
    assert np.array_equal(words(lines[0]), bits(T).reshape(-1)) and np.array_equal(words(lines[1]), bits(info).reshape(-1))
    T, info, _ = dev.multi_scale_icp(p["src"], p["dst"], sizes[:1], [50], float(v32) * 1.4, init, 1, p["dst_normals"])
    assert np.array_equal(words(lines[2]), bits(T).reshape(-1)) and np.array_equal(words(lines[3]), bits(info).reshape(-1))
    assert lines[4] == "[Misc3D Error] " + iu.NO_NORMALS
    assert "not accelerated" in lines[5]
