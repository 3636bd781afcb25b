"""m3d_color_gradient, m3d_registration_icp_colored and m3d_multi_scale_icp_colored on the MI355X against the plain-C restatement
of the contract (tests/cpp/colored_icp_ref.c, levels from tests/cpp/voxel_ref.c).  Gradients bit for bit (serial sums in a
defined order on both sides, the same solve); ICP with the bars of tests/test_gpu_icp.py: iteration counts, correspondence
arrays and fitness equal, inlier_rmse to rel 1e-9, poses to atol 1e-9 (the project's n-point bar); run-to-run and
thread-to-thread bit equality; the multi-scale call against the restatement and, bit for bit, against the public calls composed;
the Python API and the C++ mirror.  tests/test_colored_icp.py guards every input used here."""
import os
import subprocess
import threading

import numpy as np
import pytest

import colored_icp_ref_util as cu
import icp_ref_util as iu
from test_colored_icp import guarded_case
from voxel_ref_util import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return cu.ColoredRef(tmp_path_factory.mktemp("colored_icp_ref"))


@pytest.fixture(scope="module")
def dev(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device")
    return capi


@pytest.fixture(scope="module")
def multi():
    return cu.multi_case()


@pytest.fixture(scope="module")
def multi_ref(ref, multi):
    m = multi
    out = {}
    for three in (True, False):
        vs, its = iu.levels_of(m["voxel"], three)
        out[three] = ref.multi_scale(m["src"], m["src_colors"], m["dst"], m["dst_normals"], m["dst_colors"], vs, its, m["max_dist"],
                                     m["init"])
    return out


def _run(dev, c, lam=cu.LAMBDA):
    return dev.registration_icp_colored(c["src"], c["src_colors"], c["dst"], c["dst_normals"], c["dst_colors"], c["max_dist"],
                                        c["init"], lam, c["max_iteration"], want_correspondences=True)


def _exp(ref, c, lam=cu.LAMBDA):
    return ref.icp(c["src"], c["src_colors"], c["dst"], c["dst_normals"], c["dst_colors"], c["max_dist"], c["init"],
                   c["max_iteration"], lam)


def _check(got, exp):
    T, st, corr = got
    print("iterations", st["iterations"], exp["iterations"], "fitness", st["fitness"], exp["fitness"], "rmse", st["inlier_rmse"],
          exp["inlier_rmse"], "pose diff", np.abs(T - exp["T"]).max())
    assert st["iterations"] == exp["iterations"] and st["converged"] == exp["converged"]
    assert np.array_equal(corr, exp["corr"])
    assert st["fitness"] == exp["fitness"] and st["correspondences"] == exp["correspondences"]
    assert st["inlier_rmse"] == pytest.approx(exp["inlier_rmse"], rel=1e-9, abs=0)
    assert np.allclose(T, exp["T"], rtol=0, atol=1e-9)


def _same_bits_nan_apart(a, b):
    """equal bit patterns; where a value is NaN the other is NaN too (payloads apart)"""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(np.where(na, 0.0, a)), bits(np.where(nb, 0.0, b)))


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_gradient_seams_bit_for_bit(dev, ref, n):
    s = cu.seam_cloud(n)
    exp, nn, _ = ref.gradient(s["points"], s["normals"], s["colors"], s["radius"], s["max_nn"])
    # the shapes the cloud is built for are there
    P = s["points"]
    fin = np.isfinite(P).all(axis=1)
    with np.errstate(invalid="ignore"):
        d = P[:, None, :] - P[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        within = ((d2 < s["radius"] ** 2) & fin[None, :] & fin[:, None]).sum(axis=1)
    assert {0, 3, 4, 29, 30} <= set(nn.tolist())
    assert np.any(within > 30) and np.all(nn[within > 30] == 30)              # cut by max_nn
    assert np.any((within < 30) & (within >= 4) & (nn == within))             # cut by the radius
    assert d2[49, 50] == s["radius"] ** 2 and nn[49] == 1 and nn[50] == 1     # d2 == r2 is excluded
    assert nn[47] == 0 and nn[48] == 0 and not exp[47].any() and not exp[48].any()
    assert np.array_equal(P[51], P[38]) and nn[51] >= 4                       # a copy: L[0] is the original
    assert not s["normals"][5].any() and nn[5] >= 4                           # a zero normal: a singular system, solved as it is
    assert np.all(nn[53:58] == 5) and np.isnan(exp[53:58]).all()              # the NaN colour reaches its cluster ...
    assert np.isfinite(exp[:47]).all() and np.isfinite(exp[51:53]).all()      # ... and nothing else
    got = dev.color_gradient(P, s["normals"], s["colors"], s["radius"], s["max_nn"])
    bad = [k for k in range(n) if not _same_bits_nan_apart(got[k], exp[k])]
    print("rows that differ:", bad[:10], [(got[k], exp[k]) for k in bad[:3]])
    assert not bad


def test_gradient_short_lists_and_other_max_nn(dev, ref):
    """max_nn below 4 (every gradient zero), and a max_nn that is not the ICP's"""
    s = cu.seam_cloud(257)
    assert not dev.color_gradient(s["points"], s["normals"], s["colors"], s["radius"], 3).any()
    exp, nn, _ = ref.gradient(s["points"], s["normals"], s["colors"], 0.2, 7)
    assert nn.max() == 7
    assert _same_bits_nan_apart(dev.color_gradient(s["points"], s["normals"], s["colors"], 0.2, 7), exp)


@pytest.mark.parametrize("name", cu.CASES)
def test_colored_icp_matches_the_reference(dev, ref, name):
    c = cu.case(name)
    exp = _exp(ref, c)
    got = _run(dev, c)
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


@pytest.mark.parametrize("name", ["n255", "n256", "n257", "n16385"])
def test_iteration_kernel_workgroup_seams(dev, ref, name):
    """the workgroup edge (255, 256, 257 moving points) and 65 workgroup records (the 64-stride edge of the final launch)"""
    c, lam = guarded_case(name)
    assert c["max_iteration"] <= 3 and len(c["src"]) == int(name[1:])
    exp = _exp(ref, c, lam)
    assert exp["correspondences"] > 0.9 * len(c["src"])
    _check(_run(dev, c, lam), exp)


def test_lambda_one_is_point_to_plane(dev, ref):
    c, lam = guarded_case("lambda1")
    got = _run(dev, c, lam)
    _check(got, _exp(ref, c, lam))
    Tp, stp = dev.registration_icp_plane(c["src"], c["dst"], c["dst_normals"], c["max_dist"], c["init"], c["max_iteration"])
    assert np.allclose(got[0], Tp, rtol=0, atol=1e-9) and got[1]["iterations"] == stp["iterations"]


def test_lambda_zero(dev, ref):
    c, lam = guarded_case("lambda0")
    _check(_run(dev, c, lam), _exp(ref, c, lam))


def test_colour_matters(dev, ref):
    c = cu.slide_case()
    exp = _exp(ref, c)
    got = _run(dev, c)
    _check(got, exp)
    assert np.linalg.norm(got[0][:2, 3]) < np.linalg.norm(c["shift"]) / 5
    Tp, stp = dev.registration_icp_plane(c["src"], c["dst"], c["dst_normals"], c["max_dist"], c["init"], c["max_iteration"])
    assert np.array_equal(bits(Tp), bits(c["init"]))      # point-to-plane cannot see the slide


def test_deterministic_alone_and_from_two_threads(dev):
    cases = [cu.case("refine"), cu.case("duplicates")]
    alone = [_run(dev, c) for c in cases]
    for c, a in zip(cases, alone):
        again = _run(dev, c)
        assert np.array_equal(bits(again[0]), bits(a[0])) and np.array_equal(again[2], a[2])
        assert again[1]["inlier_rmse"] == a[1]["inlier_rmse"]
    out = [None, None]

    def work(k):
        out[k] = [_run(dev, cases[k]) for _ in range(3)]
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


def _multi(dev, m, vs, its):
    return dev.multi_scale_icp_colored(m["src"], m["src_colors"], m["dst"], m["dst_normals"], m["dst_colors"], vs, its, m["max_dist"],
                                       m["init"])


@pytest.mark.parametrize("three", [True, False])
def test_multi_scale_matches_the_reference(dev, multi, multi_ref, three):
    m = multi
    vs, its = iu.levels_of(m["voxel"], three)
    exp = multi_ref[three]
    T, info, levels = _multi(dev, m, vs, its)
    print([(l["n_src"], l["n_dst"], l["icp"]["iterations"], round(l["ms_down_sample"], 3), round(l["ms_icp"], 3),
            round(l["ms_information"], 3)) for l in levels], "pose diff", np.abs(T - exp["T"]).max())
    assert len(levels) == len(vs)
    for got, e in zip(levels, exp["levels"]):
        assert (got["n_src"], got["n_dst"]) == (e["n_src"], e["n_dst"])
        assert got["icp"]["iterations"] == e["iterations"] and got["icp"]["fitness"] == e["fitness"]
    assert np.allclose(T, exp["T"], rtol=0, atol=1e-9)
    assert info[5, 5] == exp["n_info"] == exp["info"][5, 5]
    assert np.abs(info - exp["info"]).max() <= 1e-9 * np.abs(exp["info"]).max()


def test_multi_scale_equals_the_public_calls_composed(dev, multi):
    m = multi
    vs, its = iu.levels_of(m["voxel"], True)
    T, info, levels = _multi(dev, m, vs, its)
    ls = dev.voxel_down_sample_multi(m["src"], vs, None, m["src_colors"])
    ld = dev.voxel_down_sample_multi(m["dst"], vs, m["dst_normals"], m["dst_colors"])
    cur = m["init"]
    for l, (s, d, it) in enumerate(zip(ls, ld, its)):
        cur, st = dev.registration_icp_colored(s["points"], s["colors"], d["points"], d["normals"], d["colors"], m["max_dist"], cur,
                                               cu.LAMBDA, it)
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

    class Cloud:
        def __init__(self, p, n, c):
            self.points, self.normals, self.colors = p, n, c
    src, dst = Cloud(m["src"], None, m["src_colors"]), Cloud(m["dst"], m["dst_normals"], m["dst_colors"])
    T, info = rec.refine_fragment_pair(src, dst, iu.MULTI_VOXEL, m["init"], rec.LocalRefineMethod.ColoredICP)
    v32 = np.float32(iu.MULTI_VOXEL)
    sizes = [float(v32), float(v32 / np.float32(2)), float(v32 / np.float32(4))]
    T2, info2, _ = dev.multi_scale_icp_colored(m["src"], m["src_colors"], m["dst"], m["dst_normals"], m["dst_colors"], sizes,
                                               [50, 30, 15], float(v32) * 1.4, m["init"])
    assert np.array_equal(bits(T), bits(T2)) and np.array_equal(bits(info), bits(info2))
    assert np.allclose(T, m["T"], rtol=0, atol=1e-3)
    To, _, lv = rec.fragment_odometry((m["src"], None, m["src_colors"]), (m["dst"], m["dst_normals"], m["dst_colors"]),
                                      iu.MULTI_VOXEL, m["init"], "colored", stats=True, lambda_geometric=0.9)
    To2, _, _ = dev.multi_scale_icp_colored(m["src"], m["src_colors"], m["dst"], m["dst_normals"], m["dst_colors"], sizes[:1], [50],
                                            float(v32) * 1.4, m["init"], 0.9)
    assert np.array_equal(bits(To), bits(To2)) and len(lv) == 1 and not np.array_equal(bits(To), bits(T))
    # the colourless ColoredICP call is refused as before; the colourless methods do not read the colours
    with pytest.raises(RuntimeError, match="not accelerated"):
        rec.refine_fragment_pair(m["src"], (m["dst"], m["dst_normals"]), iu.MULTI_VOXEL, m["init"], rec.LocalRefineMethod.ColoredICP)
    Tp, _ = rec.fragment_odometry(src, dst, iu.MULTI_VOXEL, m["init"])
    Tp2, _ = rec.fragment_odometry(m["src"], (m["dst"], m["dst_normals"]), iu.MULTI_VOXEL, m["init"])
    assert np.array_equal(bits(Tp), bits(Tp2))
    c = cu.case("small")
    Tc, st = m3d.registration_colored_icp((c["src"], None, c["src_colors"]), (c["dst"], c["dst_normals"], c["dst_colors"]),
                                          c["max_dist"], c["init"])
    Td, std = _run(dev, c)[:2]
    assert np.array_equal(bits(Tc), bits(Td)) and st["iterations"] == std["iterations"]


def test_cpp_mirror(dev, tmp_path):
    exe = str(tmp_path / "colored_icp_mirror")
    lib = os.path.join(ROOT, "misc3d_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_colored_icp_mirror.cpp"), "-o", exe, "-L", lib, "-lmisc3d_amd",
                    "-lpthread", "-Wl,-rpath," + lib], check=True)
    p = iu.icp_pair(6001, seed=31)
    sc, dc = cu.colors_of(p)
    v = 0.05
    init = iu.offset_pose(p["T"], 1.0, (0.01, -0.005, 0.008))
    blob = tmp_path / "pair.bin"
    blob.write_bytes(np.array([len(p["src"]), len(p["dst"])], dtype=np.uint64).tobytes() + p["src"].tobytes() + sc.tobytes()
                     + p["dst"].tobytes() + p["dst_normals"].tobytes() + dc.tobytes() + np.ascontiguousarray(init).tobytes()
                     + np.float64(v).tobytes())
    r = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")

    def words(line):
        return np.array([int(t, 16) for t in line.split()], dtype=np.uint64)
    v32 = np.float32(v)
    sizes = [float(v32), float(v32 / np.float32(2)), float(v32 / np.float32(4))]
    T, info, _ = dev.multi_scale_icp_colored(p["src"], sc, p["dst"], p["dst_normals"], dc, sizes, [50, 30, 15], float(v32) * 1.4, init)
    assert np.array_equal(words(lines[0]), bits(T).reshape(-1)) and np.array_equal(words(lines[1]), bits(info).reshape(-1))
    assert "not accelerated" in lines[2]
