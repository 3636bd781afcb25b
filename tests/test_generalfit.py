"""GeneralFit (RefineModel's plane and sphere refinement), the part that needs no GPU: the exact references of
tests/generalfit_ref_util.py on cases worked out by hand, the oracle against them on every input family of the GPU tests, the
families' own properties (which plane cases the closed form leaves undecided, which make it fail), the proof that the bound of
tests/test_gpu_generalfit.py can fail -- the arithmetic of the fused sums with the provisional centre at a minimal sphere's
CENTRE breaks it, with the centre among the inliers it holds -- and the closed forms of misc3d_amd/csrc/m3d_generalfit_fp.hpp,
compiled with g++ and fed exactly summed moments (tests/cpp/test_generalfit_fp.cpp).

Measured here (seed 11), err / max(err(oracle), F), M = 32:
                        oracle err   two-pass   fused, c0 an inlier   fused, c0 = the winner's minimal centre
  sphere_full              8e-15       0.03          0.01                 0.0
  sphere_cap20             5e-15       0.07          0.07                 1.0
  sphere_cap10             3e-15       6.1           1.9                  732
  sphere_cap5_r5           1e-14       3.3           5.6                  799
  sphere_cap10_at_1e3      2e-08       0.00          0.00                 0.0
  sphere_cap5_r5_at_1e3    1e-09       0.00          0.00                 0.2
So the centre-based sums lose (radius / extent)^3 as predicted, but the bound -- relative to the ORACLE's error -- sees it on
the 10 and 5 degree caps only: on the 20 degree cap the loss is 27 units in the last place, the oracle's own size, and on
the translated caps the oracle (Householder QR of the uncentred system) is itself off by 1e-9 .. 2e-8, more than any
provisional centre loses.  A cap 1e5 away is beyond RANSAC altogether (Case.ransac).  The device agrees (header of
tests/test_gpu_generalfit.py): 1748 and 680 on the two caps with the parent's sums, 3.8 and 2.3 with the sample's centroid.
"""
import os
import subprocess

import numpy as np
import pytest
from fractions import Fraction

import generalfit_ref_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53


# ---------------------------------------------------------------------------------------------- the references, by hand
def test_exact_plane_by_hand():
    # the unit square in z = 0: xx = yy = 1, everything else 0 -> det_z = 1, the others 0
    ex = gu.exact_plane([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
    assert ex["ok"] and ex["branch"] == 2 and ex["params"] == (0, 0, 1, 0) and ex["gap"] == 1.0 and ex["norm"] == 1
    # 2 x + 3 y + 6 z = 6 (|(2, 3, 6)| = 7): the z determinant is the largest, c > 0
    ex = gu.exact_plane([[3, 0, 0], [0, 2, 0], [0, 0, 1], [3, 2, -1]])
    assert ex["ok"] and ex["branch"] == 2
    assert gu.err([2 / 7, 3 / 7, 6 / 7, -6 / 7], ex["params"]) < 2 * EPS       # (the doubles nearest to the sevenths)
    assert max(abs(e - t) for e, t in zip(ex["params"], (Fraction(2, 7), Fraction(3, 7), Fraction(6, 7), Fraction(-6, 7)))) < Fraction(1, 10 ** 55)
    # the same plane with x the largest component: 6 x + 3 y + 2 z = 6 -> branch 0, a > 0
    ex = gu.exact_plane([[1, 0, 0], [0, 2, 0], [0, 0, 3], [-1, 2, 3]])
    assert ex["branch"] == 0 and max(abs(e - t) for e, t in zip(ex["params"], (Fraction(6, 7), Fraction(3, 7), Fraction(2, 7), Fraction(-6, 7)))) < Fraction(1, 10 ** 55)
    # x = y with x, y the same multiset: det_x == det_y exactly -> not `det_x > det_y`, branch 1, b > 0 and a < 0
    ex = gu.exact_plane([[0, 0, 0], [1, 1, 0], [0, 0, 1], [1, 1, 1]])
    assert ex["branch"] == 1 and ex["gap"] == 0.0 and len(ex["alternatives"]) == 2
    assert float(ex["params"][0]) < 0 < float(ex["params"][1]) and abs(float(ex["params"][1]) - 0.5 ** 0.5) < 2 * EPS
    # the failure test: norm = (1e-2)^4 = 1e-8 is no failure (`<`), a hair smaller is; fewer than three points fail
    sq = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=np.float64)
    assert gu.exact_plane(sq * 2.0 ** -6)["ok"] and float(gu.exact_plane(sq * 2.0 ** -6)["norm"]) == 2.0 ** -24
    assert not gu.exact_plane(sq * 2.0 ** -7)["ok"] and float(gu.exact_plane(sq * 2.0 ** -7)["norm"]) == 2.0 ** -28
    assert not gu.exact_plane(sq[:2])["ok"] and gu.exact_plane(sq[:3])["ok"]


def test_exact_sphere_by_hand():
    c = np.array([1.0, 2.0, 3.0])
    six = np.array([c + s * 2.0 * e for e in np.eye(3) for s in (1, -1)])
    ex = gu.exact_sphere(six)
    assert ex["ok"] and ex["params"] == (1, 2, 3, 2)
    # four points determine their sphere: centre (1, 1, 1), radius sqrt 3
    ex = gu.exact_sphere([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 2]])
    assert ex["params"][:3] == (1, 1, 1) and abs(ex["params"][3] ** 2 - 3) < Fraction(1, 10 ** 55)
    # a least-squares case: the six points above and the centre's mirror pair pulled in by 1 along x: by symmetry the centre
    # stays, radius^2 = mean |p - c|^2 = (6 * 4 + 2 * 1) / 8
    eight = np.concatenate([six, [c + [1, 0, 0], c - [1, 0, 0]]])
    ex = gu.exact_sphere(eight)
    assert ex["params"][:3] == (1, 2, 3) and abs(ex["params"][3] ** 2 - Fraction(26, 8)) < Fraction(1, 10 ** 55)
    assert not gu.exact_sphere(six[:3])["ok"] and gu.exact_sphere(six[:4])["singular"]      # (four coplanar points)
    assert gu.err([1.0, 2.0, 3.0, 2.0 + 2.0 ** -40], gu.exact_sphere(six)["params"]) == 2.0 ** -40


def test_emulations_by_hand():
    six = np.array([[3, 2, 3], [-1, 2, 3], [1, 4, 3], [1, 0, 3], [1, 2, 5], [1, 2, 1]], dtype=np.float64)
    for c0 in (six[0], [0.0, 0.0, 0.0]):
        ok, p = gu.emulate_fused(six, c0, gu.SPHERE)
        assert ok and np.array_equal(p, [1, 2, 3, 2])
    ok, p = gu.emulate_two_pass(six, gu.SPHERE)
    assert ok and np.array_equal(p, [1, 2, 3, 2])
    sq = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1]], dtype=np.float64)
    for ok, p in (gu.emulate_fused(sq, sq[3], gu.PLANE), gu.emulate_two_pass(sq, gu.PLANE)):
        assert ok and np.array_equal(p, [0, 0, 1, -1])


# ---------------------------------------------------------------------------------------------- the oracle on every family
def _oracle_error_bound(p):
    """What an fp64 evaluation in the oracle's order may lose (the oracle is the yardstick of the GPU bound, so its own error is
    bounded here from the conditioning of its problem, not from anything the code under test computes):
    plane -- serial sums of n terms, the closed form amplifies by the in-plane moment ratio; sphere -- Householder QR of the
    UNCENTRED n x 4 system A = [2x 2y 2z 1], b = |p|^2: forward error <= c n eps max|b| / sigma_min(A)."""
    pts, n = p.points, len(p.points)
    scale = max(1.0, float(np.abs(pts).max()))
    if p.case.kind == gu.PLANE:
        lam = np.linalg.eigvalsh(np.cov((pts - pts.mean(axis=0)).T))
        return 8.0 * n * EPS * scale * float(lam[2] / lam[1])
    A = np.hstack([2.0 * pts, np.ones((n, 1))])
    return 64.0 * n * EPS * float((pts * pts).sum(axis=1).max()) / float(np.linalg.svd(A, compute_uv=False)[-1])


@pytest.mark.parametrize("name", list(gu.FAMILIES))
def test_oracle_agrees_with_the_exact_reference(orc, name):
    p = gu.prepare(name, orc)
    k = p.case.kind
    assert len(p.case.pts) <= 8000
    if p.case.ransac:
        assert p.fit.best_index >= 0
    tiny = {"sphere_4_inliers": 4, "sphere_5_inliers": 5, "sphere_6_inliers": 6, "plane_3_inliers": 3, "plane_4_inliers": 4}
    if name in tiny:
        assert len(p.inliers) == tiny[name]
    elif p.case.ransac:
        assert len(p.inliers) >= 2500        # RANSAC has selected the structure
    ok_o, par_o = (orc.plane_general_fit if k == gu.PLANE else orc.sphere_general_fit)(p.points)
    assert ok_o == bool(p.oracle_ok)
    if name in gu.FAIL_FAMILIES:
        # the closed form fails in exact arithmetic, a factor of 10 away from the test: the oracle fails too and RefineModel
        # leaves the best minimal model in place
        assert not p.exact["ok"] and float(p.exact["norm"]) < 1e-9 and not ok_o
        assert np.array_equal(p.oracle_params, p.minimal)
        print(f"{name}: exact norm {float(p.exact['norm']):.3e} -> GeneralFit fails")
        return
    assert p.exact["ok"] and ok_o and np.array_equal(par_o, p.oracle_params)
    if k == gu.PLANE:
        assert float(p.exact["norm"]) > 1e-7
    print(f"{name}: inliers {len(p.inliers)}  err(oracle) {p.oracle_err:.3e}  F {p.F:.3e}  bound on the oracle {_oracle_error_bound(p):.3e}")
    assert p.oracle_err <= _oracle_error_bound(p)


def test_cluster_families_sit_a_decade_on_either_side_of_the_failure_test(orc):
    below, above = gu.prepare("plane_cluster_norm_below", orc), gu.prepare("plane_cluster_norm_above", orc)
    assert below.exact["norm"] < Fraction(1, 10 ** 9) and above.exact["norm"] > Fraction(1, 10 ** 7)


def test_no_ransac_fit_selects_a_cap_1e5_away(orc):
    """why two families reach GeneralFit through RefineModel on the true model only (Case.ransac)"""
    for name in gu.FAMILIES:
        c = gu.family(name, orc)
        if not c.ransac:
            o = orc.fit(c.kind, c.pts, None, thr=c.thr, max_iter=c.max_iter, prob=c.prob, seed=c.seed)
            assert len(o.inliers) < 100, name
            assert len(gu.prepare(name, orc).inliers) >= 2500


def test_undecided_plane_cases_are_the_tie_families(orc):
    """A plane case is undecided when the exact relative gap between the two largest determinants is below 1e-9: rounding then
    picks the branch.  Outside the two tie families there is no such case."""
    undecided = []
    for name in gu.PLANE_FAMILIES:
        p = gu.prepare(name, orc)
        if p.exact["gap"] is not None:
            print(f"{name}: gap {p.exact['gap']:.3e} branch {p.exact['branch']}")
            if p.exact["gap"] < gu.UNDECIDED_GAP:
                undecided.append(name)
    assert sorted(undecided) == sorted(gu.TIE_FAMILIES)
    for name in gu.TIE_FAMILIES:        # the mirror construction makes the tie exact, and the two branches differ by more than the sign
        p = gu.prepare(name, orc)
        assert p.exact["gap"] == 0.0 and len(p.exact["alternatives"]) == 2
        assert gu.err_mod_sign([float(v) for v in p.exact["alternatives"][0]], p.exact["alternatives"][1]) > 1e3 * p.bound


# ---------------------------------------------------------------------------------------------- the bound can fail
@pytest.mark.parametrize("name", [n for n in gu.FAMILIES if n not in gu.FAIL_FAMILIES])
def test_emulated_sums_about_an_inlier_and_about_the_mean_meet_the_bound(orc, name):
    """the arithmetic of both device paths, in numpy fp64 with a free summation order: at least a factor of 4 inside M"""
    p = gu.prepare(name, orc)
    k = p.case.kind
    ok2, two = gu.emulate_two_pass(p.points, k)
    r2 = gu.ratio(p, two)
    line = f"{name}: two-pass {r2:.2f}"
    assert ok2 and r2 <= gu.M_BOUND / 4
    for c0 in (p.points[0], p.points[len(p.points) // 2], p.points[-1]):
        okf, fused = gu.emulate_fused(p.points, c0, k)
        rf = gu.ratio(p, fused)
        line += f"  fused about an inlier {rf:.2f}"
        assert okf and rf <= gu.M_BOUND / 4
    if p.case.ransac:      # the provisional centre the device takes, against the bound itself
        okf, fused = gu.emulate_fused(p.points, gu.device_c0(p), k)
        e = gu.err_case(k, fused, p.exact)
        line += f"  fused about the device's c0 {gu.ratio(p, fused):.2f} (err {e:.2e}, bound {p.bound:.2e})"
        assert okf and e <= p.bound
    print(line)


@pytest.mark.parametrize("name", [n for n in gu.CAP_FAMILIES if "1e5" not in n])
def test_emulated_sums_about_the_minimal_centre_break_the_bound(orc, name):
    """the parent's arithmetic: the sphere's raw moments about the winning minimal model's CENTRE.  On the 10 and 5 degree
    caps it misses the bound by more than a factor of 4 beyond M; on the others it cannot be told from the oracle (header)."""
    p = gu.prepare(name, orc)
    ok, par = gu.emulate_fused(p.points, p.minimal[:3], gu.SPHERE)
    r = gu.ratio(p, par)
    ok_i, par_i = gu.emulate_fused(p.points, gu.device_c0(p), gu.SPHERE)      # what the library uses: the centroid of the sample
    ri = gu.ratio(p, par_i)
    print(f"{name}: c0 = minimal centre {r:.1f}   c0 = centroid of the sample {ri:.2f}   (M = {gu.M_BOUND:g})")
    assert all(i in p.inliers for i in p.sample) and ri <= gu.M_BOUND / 4
    if name in gu.DISCRIMINATING_CAPS:
        assert r >= 4 * gu.M_BOUND
        assert gu.err(par, p.exact["params"]) > p.bound


# ---------------------------------------------------------------------------------------------- the closed forms on the host
def _hex(v):
    return np.float64(v).view(np.uint64).item().to_bytes(8, "big").hex()


def test_closed_forms_on_exact_moments(orc, tmp_path):
    """tests/cpp/test_generalfit_fp.cpp compiles m3d_generalfit_fp.hpp -- the text the library compiles -- with g++.  Its input:
    per family the raw moments about the first inlier and the centred moments, each summed EXACTLY and rounded once; on the
    discriminating caps also the raw moments about the winner's minimal centre.  With exact sums the closed forms meet the
    bound (so a miss on the GPU is the sums'), and the shift from a centre one radius away breaks it on its own (CENTRE_EXACT:
    the parent lost bits in the formula AND, ten times as many, in sums whose terms are a radius large)."""
    exe = str(tmp_path / "test_generalfit_fp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "test_generalfit_fp.cpp"),
                    "-o", exe], check=True, capture_output=True)
    lines, what = [], []
    for name in gu.FAMILIES:
        p = gu.prepare(name, orc)
        k, n = p.case.kind, len(p.points)
        c0s = [("inlier", p.points[0])]
        if name in gu.DISCRIMINATING_CAPS:
            c0s.append(("centre", p.minimal[:3]))
        for tag, c0 in c0s:
            raw = gu.exact_raw_moments(p.points, c0)
            lines.append(f"{k} 0 {n} " + " ".join(_hex(v) for v in list(c0) + raw))
            what.append((name, tag))
        mean, cen = gu.exact_centred_moments(p.points)
        lines.append(f"{k} 1 {n} " + " ".join(_hex(v) for v in mean + cen))
        what.append((name, "centred"))
    src = tmp_path / "moments.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(what)
    for (name, tag), line in zip(what, out):
        p = gu.prepare(name, orc)
        f = line.split()
        ok, par = int(f[0]), np.array([int(w, 16) for w in f[1:]], dtype=np.uint64).view(np.float64)
        if name in gu.FAIL_FAMILIES:
            assert ok == 0, (name, tag)
            continue
        rr = gu.ratio(p, par)
        print(f"{name} [{tag}]: {rr:.2f}")
        # the emulation in Python floats is the same arithmetic: bit for bit
        if tag == "centred":
            mean, cen = gu.exact_centred_moments(p.points)
            ok_e, par_e = gu._closed_form(p.case.kind, mean, cen, len(p.points))
            assert ok_e and np.array_equal(par_e, par), (name, tag)
        if tag == "centre":
            assert ok == 1 and rr > gu.M_BOUND, (name, tag, rr)
        else:
            assert ok == 1 and rr <= gu.M_BOUND / 4, (name, tag, rr)
