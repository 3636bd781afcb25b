"""Coloured ICP, the part that needs no GPU: the plain-C restatement (tests/cpp/colored_icp_ref.c) on a hand case and against
an independent numpy restatement, the guard on every input the GPU tests use, the case in which only the colours can see the
motion, the 3 x 3 and 6 x 6 solves of m3d_icp_fp.hpp compiled on the host, and the argument checks of the three entry points
(decided before any device work)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import colored_icp_ref_util as cu
import icp_ref_util as iu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return cu.ColoredRef(tmp_path_factory.mktemp("colored_icp_ref"))


@pytest.fixture(scope="module")
def tiny():
    p = iu.icp_pair(60, seed=3)
    c = dict(src=p["src"], dst=p["dst"], T=p["T"])
    sc, dc = cu.colors_of(c)
    return p["src"], sc, p["dst"], p["dst_normals"], dc


def _args(c):
    return c["src"], c["src_colors"], c["dst"], c["dst_normals"], c["dst_colors"], c["max_dist"], c["init"], c["max_iteration"]


def test_linear_ramp_by_hand(ref):
    """I = a x + b y + c on a regular planar grid with unit normal z: the gradient is (a, b, 0) at interior points whatever 30
    neighbours the list holds, and (0, 0, 0) where the list has fewer than 4 entries"""
    r = cu.ramp_case()
    g, nn, _ = ref.gradient(r["points"], r["normals"], r["colors"], r["radius"])
    assert r["interior"].sum() >= 20 and np.all(nn[r["interior"]] >= 4)
    assert np.abs(g[r["interior"]] - r["gradient"]).max() <= 1e-12
    assert np.all(nn[r["lone"]] < 4) and not g[r["lone"]].any()


# (refine / no_convergence are "small"'s generator at 6001 points: the numpy restatement would take a quarter of a minute there)
FAMILIES = ("small", "duplicates", "nonfinite", "no_correspondences", "identity_init", "slide")


def _family(name):
    return cu.slide_case() if name == "slide" else cu.case(name)


@pytest.mark.parametrize("name", FAMILIES)
def test_c_reference_matches_the_numpy_restatement(ref, name):
    c = _family(name)
    g, nn, _ = ref.gradient(c["dst"], c["dst_normals"], c["dst_colors"], 2.0 * c["max_dist"])
    with np.errstate(invalid="ignore"):
        gn, cond = cu.gradient_numpy(c["dst"], c["dst_normals"], c["dst_colors"], 2.0 * c["max_dist"])
    well = (nn >= 4) & (cond <= 1e8)
    left_out = int(((nn >= 4) & ~well).sum())
    print(name, "points left out of the gradient comparison:", left_out, "of", len(nn))
    assert left_out < 0.01 * len(nn)
    assert not g[nn < 4].any() and not gn[nn < 4].any()
    scale = np.abs(gn[well]).max(axis=1, keepdims=True)
    assert np.all(np.abs(g[well] - gn[well]) <= 1e-9 * scale)
    a = ref.icp(*_args(c))
    with np.errstate(invalid="ignore"):
        b = cu.icp_numpy(*_args(c))
    assert a["iterations"] == b["iterations"] and a["converged"] == b["converged"]
    assert np.array_equal(a["corr"], b["corr"]) and a["fitness"] == b["fitness"]
    assert np.allclose(a["T"], b["T"], rtol=0, atol=1e-9)


def _guard(a, b):
    assert a["iterations"] == b["iterations"] and np.array_equal(a["corr"], b["corr"])


GUARDED = list(cu.CASES) + ["slide", "n255", "n256", "n257", "n16385", "lambda1", "lambda0"]


def guarded_case(name):
    """every input of tests/test_gpu_colored_icp.py -> (case, lambda)"""
    if name == "slide":
        return cu.slide_case(), cu.LAMBDA
    if name[0] == "n" and name[1:].isdigit():
        return cu.sized_case(int(name[1:])), cu.LAMBDA
    if name.startswith("lambda"):
        c = cu.case("small")
        c["max_iteration"] = 3
        return c, float(name[6:])
    return cu.case(name), cu.LAMBDA


@pytest.mark.parametrize("name", GUARDED)
def test_input_guard_single_level(ref, name):
    """the restatement summed in ascending and in descending index order gives the same iteration count and correspondences
    on every input the GPU tests use: the order of the sums, which the device fixes differently, decides nothing on it"""
    c, lam = guarded_case(name)
    _guard(ref.icp(*_args(c), lam=lam, order=1), ref.icp(*_args(c), lam=lam, order=-1))


@pytest.mark.parametrize("three", [True, False])
def test_input_guard_multi_scale(ref, three):
    m = cu.multi_case()
    vs, its = iu.levels_of(m["voxel"], three)
    a = ref.multi_scale(m["src"], m["src_colors"], m["dst"], m["dst_normals"], m["dst_colors"], vs, its, m["max_dist"], m["init"])
    b = ref.multi_scale(m["src"], m["src_colors"], m["dst"], m["dst_normals"], m["dst_colors"], vs, its, m["max_dist"], m["init"],
                        order=-1)
    for x, y in zip(a["levels"], b["levels"]):
        _guard(x, y)
    assert a["n_info"] == b["n_info"] and a["levels"][0]["iterations"] >= 3
    assert np.allclose(a["T"], m["T"], rtol=0, atol=1e-3)


def test_colour_matters(ref):
    """a textured plane slid inside itself: point-to-plane's JTJ is singular (the update is the identity, the pose stays the
    initial one); the coloured restatement recovers the slide to better than a fifth of the initial in-plane error"""
    c = cu.slide_case()
    p = ref.plain.icp(c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"], c["dst_normals"])
    assert np.array_equal(p["T"], c["init"]) and p["iterations"] == 1
    r = ref.icp(*_args(c))
    before, after = np.linalg.norm(c["shift"]), np.linalg.norm(r["T"][:2, 3])
    print("in-plane error", before, "->", after, "iterations", r["iterations"])
    assert after < before / 5 and r["iterations"] >= 2
    assert np.abs(r["T"][:3, :3] - np.eye(3)).max() < 1e-3 and abs(r["T"][2, 3]) < 1e-9


def test_ldlt_at_both_sizes_on_the_host(tmp_path):
    """tests/cpp/test_ldlt_sizes.cpp compiles misc3d_amd/csrc/m3d_icp_fp.hpp with g++: the 3 x 3 solve against numpy on
    well-conditioned systems to rel 1e-12; the 6 x 6 solve bit-equal to what it gave before it became a template"""
    exe = str(tmp_path / "test_ldlt_sizes")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "test_ldlt_sizes.cpp"),
                    "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe, "six"], capture_output=True, text=True, timeout=60)
    with open(os.path.join(ROOT, "tests", "golden", "icp_ldlt6_digests.txt")) as f:
        assert r.returncode == 0 and r.stdout.split() == f.read().split()
    rng = np.random.default_rng(5)
    B = rng.normal(size=(500, 5, 3))
    A = np.einsum("nki,nkj->nij", B, B) + 0.5 * np.eye(3)          # condition numbers of a few tens
    A[::7, 0, 0] += 40.0                                           # (the pivot is not always the first diagonal entry ...)
    A[3::7, 2, 2] += 40.0                                          # (... nor the same one)
    b = rng.normal(size=(500, 3))
    (tmp_path / "in.bin").write_bytes(np.concatenate([A.reshape(500, 9), b], axis=1).tobytes())
    assert subprocess.run([exe, "three", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], timeout=60).returncode == 0
    x = np.fromfile(tmp_path / "out.bin").reshape(500, 3)
    want = np.linalg.solve(A, b[:, :, None])[:, :, 0]
    assert np.all(np.abs(x - want) <= 1e-12 * np.abs(want).max(axis=1, keepdims=True))


def test_symbols_exported(capi):
    for name in ("m3d_color_gradient", "m3d_registration_icp_colored", "m3d_multi_scale_icp_colored"):
        assert hasattr(capi.lib(), name), name


def test_argument_checks_need_no_gpu(capi, tiny):
    src, sc, dst, nrm, dc = tiny
    init = iu.offset_pose(np.eye(4), 3.0, (0.1, 0.2, 0.3))
    L = capi.lib()

    def refused(text, *a, **kw):
        with pytest.raises(capi.M3DError) as e:
            capi.registration_icp_colored(*a, **kw)
        assert e.value.code == capi.ERR_INVALID_ARG and str(e.value) == "[Misc3D Error] " + text

    for d in (0.0, -1.0, float("nan")):
        refused(iu.INVALID_DISTANCE, src, sc, dst, nrm, dc, d)
    refused(iu.INVALID_DISTANCE, src, None, dst, None, None, 0.0, lambda_geometric=2.0)      # the distance is checked first
    refused(iu.NO_NORMALS, src, sc, dst, None, dc, 0.05)
    refused(iu.NO_NORMALS, src, None, dst, None, None, 0.05, lambda_geometric=2.0)           # ... then the normals
    refused(cu.NO_COLORS, src, None, dst, nrm, dc, 0.05)
    refused(cu.NO_COLORS, src, sc, dst, nrm, None, 0.05, lambda_geometric=2.0)               # ... then the colours
    for lam in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        refused(cu.BAD_LAMBDA, src, sc, dst, nrm, dc, 0.05, lambda_geometric=lam)
    # the outputs of a refused call: the initial pose, zeroed stats
    T, st = np.full(16, 7.0), capi.IcpStats()
    st.iterations = 9
    Ti = init.reshape(16).copy()
    assert L.m3d_registration_icp_colored(capi._p(src), None, len(src), capi._p(dst), capi._p(nrm), capi._p(dc), len(dst), 0.05,
                                          0.968, capi._p(Ti), 30, 1e-6, 1e-6, 0, capi._p(T), C.cast(C.byref(st), C.c_void_p),
                                          None) == capi.ERR_INVALID_ARG
    assert np.array_equal(T, Ti) and st.iterations == 0
    assert L.m3d_registration_icp_colored(capi._p(src), capi._p(sc), len(src), capi._p(dst), capi._p(nrm), capi._p(dc), len(dst),
                                          0.05, 0.968, None, 30, 1e-6, 1e-6, 0, None, None, None) == capi.ERR_INVALID_ARG
    # an empty cloud is no error and needs no device: the pose is the initial one, the first repeat meets both criteria
    e3 = np.zeros((0, 3))
    T, st = capi.registration_icp_colored(e3, e3, dst, nrm, dc, 0.05, init)
    assert np.array_equal(T, init) and st["iterations"] == 1 and st["converged"] == 1 and st["fitness"] == 0.0
    T, st, corr = capi.registration_icp_colored(src, sc, e3, e3, e3, 0.05, want_correspondences=True)
    assert np.array_equal(T, np.eye(4)) and np.all(corr == -1) and len(corr) == len(src)
    assert capi.color_gradient(e3, e3, e3, 0.1).shape == (0, 3)
    # m3d_color_gradient
    for kw, text in ((dict(max_nn=0), "max_nn"), (dict(max_nn=129), "max_nn"), (dict(radius=-1.0), "radius"),
                     (dict(radius=float("nan")), "radius"), (dict(dst_normals=None), iu.NO_NORMALS),
                     (dict(dst_colors=None), "no colors")):
        a = dict(dst=dst, dst_normals=nrm, dst_colors=dc, radius=0.1, max_nn=30)
        a.update(kw)
        with pytest.raises(capi.M3DError) as e:
            capi.color_gradient(**a)
        assert e.value.code == capi.ERR_INVALID_ARG and text in str(e.value)


def test_multi_scale_argument_checks_need_no_gpu(capi, tiny):
    src, sc, dst, nrm, dc = tiny

    def fails(msg, *a, **kw):
        with pytest.raises(capi.M3DError) as e:
            capi.multi_scale_icp_colored(*a, **kw)
        assert e.value.code == capi.ERR_INVALID_ARG and msg in str(e.value), str(e.value)

    fails("no levels", src, sc, dst, nrm, dc, [], [], 0.07)
    fails(iu.NO_NORMALS, src, sc, dst, None, dc, [0.05], [50], 0.07)
    fails(cu.NO_COLORS, src, None, dst, nrm, dc, [0.05], [50], 0.07)
    fails(cu.NO_COLORS, src, sc, dst, nrm, None, [0.05], [50], 0.07)
    fails(cu.BAD_LAMBDA, src, sc, dst, nrm, dc, [0.05], [50], 0.07, lambda_geometric=1.5)
    fails("[VoxelDownSample] voxel_size <= 0.", src, sc, dst, nrm, dc, [0.05, 0.0], [50, 30], 0.07)
    fails(iu.INVALID_DISTANCE, src, sc, dst, nrm, dc, [0.05], [50], 0.0)
    L = capi.lib()
    init = iu.offset_pose(np.eye(4), 3.0, (0.1, 0.2, 0.3)).reshape(16).copy()
    T, info = np.full(16, 7.0), np.full(36, 7.0)
    assert L.m3d_multi_scale_icp_colored(capi._p(src), None, None, len(src), capi._p(dst), capi._p(nrm), capi._p(dc), len(dst), None,
                                         None, 0, 0.07, 0.968, capi._p(init), 0, capi._p(T), capi._p(info),
                                         None) == capi.ERR_INVALID_ARG
    assert np.array_equal(T, init) and not info.any()
    # method 2 of the colourless call keeps refusing
    with pytest.raises(capi.M3DError, match="not accelerated"):
        capi.multi_scale_icp(src, dst, [0.05], [50], 0.07, method=capi.REFINE_COLORED_ICP, dst_normals=nrm)


def test_python_api_argument_checks_need_no_gpu(tiny):
    import misc3d_amd as m3d
    src, sc, dst, nrm, dc = tiny
    rec = m3d.reconstruction
    with pytest.raises(RuntimeError, match="requires colors"):
        m3d.registration_colored_icp(src, (dst, nrm, dc), 0.05)
    with pytest.raises(RuntimeError, match="require pre-computed normal"):
        m3d.registration_colored_icp((src, None, sc), dst, 0.05)
    with pytest.raises(RuntimeError, match="lambda_geometric"):
        m3d.registration_colored_icp((src, None, sc), (dst, nrm, dc), 0.05, lambda_geometric=-0.5)

    class Cloud:
        def __init__(self, p, n, c):
            self.points, self.normals, self.colors = p, n, c
    with pytest.raises(RuntimeError, match="lambda_geometric"):
        rec.refine_fragment_pair(Cloud(src, None, sc), Cloud(dst, nrm, dc), 0.05, method=rec.LocalRefineMethod.ColoredICP,
                                 lambda_geometric=7.0)
    with pytest.raises(RuntimeError, match="voxel_size <= 0"):
        rec.fragment_odometry((src, None, sc), (dst, nrm, dc), 0.0, method="colored")
    # a cloud without colours on either side: the call does what it did before
    with pytest.raises(RuntimeError, match="not accelerated"):
        rec.refine_fragment_pair((src, None, sc), (dst, nrm), 0.05, method="colored")
    with pytest.raises(RuntimeError, match="not accelerated"):
        rec.fragment_odometry(src, Cloud(dst, nrm, dc), 0.05, method=rec.LocalRefineMethod.ColoredICP)
