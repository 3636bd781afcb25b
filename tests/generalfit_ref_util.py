"""Exact references for GeneralFit (include/misc3d/common/ransac.h:164-213, 296-330), fp64 emulations of the two device
paths that produce its sums, and the input families of tests/test_generalfit.py and tests/test_gpu_generalfit.py.

exact_plane / exact_sphere use the standard library only.  Every double is a dyadic rational: the coordinates are brought to
one power-of-two denominator, the sums are taken over Python integers (the numerators: sums of fractions with a common
denominator) and leave as fractions.Fraction; the determinants, the 3 x 3 solve and the parameters are Fractions; the two
square roots come from `decimal` at 60 digits.  Nothing here rounds to 53 bits before the caller does.
"""
from __future__ import annotations

import decimal
from fractions import Fraction

import numpy as np

PLANE, SPHERE = 0, 1
_PREC = 60
EPS_FAIL = Fraction(1.0e-8)      # `norm < 1e-8` (ransac.h:204): the double constant, taken exactly
UNDECIDED_GAP = 1e-9             # a plane case is "undecided" when the two largest determinants are closer than this (relative)


# ------------------------------------------------------------------------------------------------ exact arithmetic
def _sqrt(fr: Fraction) -> Fraction:
    """sqrt of a non-negative Fraction to 60 significant digits, as a Fraction"""
    with decimal.localcontext() as ctx:
        ctx.prec = _PREC
        d = (decimal.Decimal(fr.numerator) / decimal.Decimal(fr.denominator)).sqrt()
    return Fraction(d)


def _scaled_ints(points):
    """(n x 3 Python ints X, D) with points[i][k] == X[i][k] / D exactly, D a power of two"""
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    if not np.isfinite(pts).all():
        raise ValueError("non-finite coordinate")
    ratios = [[float(v).as_integer_ratio() for v in p] for p in pts]
    D = max((d for p in ratios for _, d in p), default=1)
    return [[num * (D // den) for num, den in p] for p in ratios], D


def _centred(points):
    """n, mean (3 Fractions), R (n x 3 ints) and scale with r_i = p_i - mean == R_i / scale exactly"""
    X, D = _scaled_ints(points)
    n = len(X)
    S = [sum(p[k] for p in X) for k in range(3)]
    mean = [Fraction(S[k], n * D) for k in range(3)]
    R = [[n * p[k] - S[k] for k in range(3)] for p in X]
    return n, mean, R, n * D


def exact_plane(points):
    """The reference's closed form (ransac.h:164-211) evaluated exactly: centred covariance sums, the three determinants, the
    branch by `det_x > det_y && det_x > det_z` / `det_y > det_z`, the `norm < 1e-8` failure.
    -> dict(ok, params (4 Fractions, None when it fails), norm (Fraction), gap (relative gap between the two largest
    determinants, float), branch (0, 1, 2), alternatives (the exact parameters of every branch within UNDECIDED_GAP))"""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if len(pts) < 3:
        return dict(ok=False, params=None, norm=None, gap=None, branch=None, alternatives=[])
    n, mean, R, sc = _centred(pts)
    s2 = sc * sc
    xx = Fraction(sum(r[0] * r[0] for r in R), s2)
    xy = Fraction(sum(r[0] * r[1] for r in R), s2)
    xz = Fraction(sum(r[0] * r[2] for r in R), s2)
    yy = Fraction(sum(r[1] * r[1] for r in R), s2)
    yz = Fraction(sum(r[1] * r[2] for r in R), s2)
    zz = Fraction(sum(r[2] * r[2] for r in R), s2)
    det_x = yy * zz - yz * yz
    det_y = xx * zz - xz * xz
    det_z = xx * yy - xy * xy
    dets = (det_x, det_y, det_z)
    vectors = ((det_x, xz * yz - xy * zz, xy * yz - xz * yy), (xz * yz - xy * zz, det_y, xy * xz - yz * xx),
               (xy * yz - xz * yy, xy * xz - yz * xx, det_z))
    branch = 0 if (det_x > det_y and det_x > det_z) else (1 if det_y > det_z else 2)
    d = sorted(dets, reverse=True)
    gap = float((d[0] - d[1]) / d[0]) if d[0] > 0 else 0.0

    def finish(abc):
        norm2 = abc[0] * abc[0] + abc[1] * abc[1] + abc[2] * abc[2]
        norm = _sqrt(norm2)
        if norm2 < EPS_FAIL * EPS_FAIL:
            return norm, None
        a, b, c = (v / norm for v in abc)
        return norm, (a, b, c, -(a * mean[0] + b * mean[1] + c * mean[2]))

    norm, params = finish(vectors[branch])
    # the branches a rounded evaluation may take when the comparison is undecided: every one whose determinant lies within
    # UNDECIDED_GAP of the largest.  With noisy points they are DIFFERENT planes (the closed form is exact for rank-2 moments
    # only), not one plane up to sign.
    alternatives = [finish(vectors[k])[1] for k in range(3) if d[0] > 0 and dets[k] >= d[0] * (1 - Fraction(UNDECIDED_GAP))]
    return dict(ok=params is not None, params=params, norm=norm, gap=gap, branch=branch,
                alternatives=[a for a in alternatives if a is not None])


def _det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def exact_sphere(points):
    """The least-squares solution of [2x 2y 2z 1] w = |p|^2 (ransac.h:296-330), exactly, through the centred normal equations
    2 S c' = sum r q, centre = mean + c', radius^2 = |c'|^2 + sum q / n (r = p - mean, q = |r|^2, S = sum r r^T); n < 4 fails.
    -> dict(ok, params (4 Fractions or None), singular (S has no inverse: the problem has no unique answer))"""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if len(pts) < 4:
        return dict(ok=False, params=None, singular=False)
    n, mean, R, sc = _centred(pts)
    s2, s3 = sc * sc, sc * sc * sc
    Q = [r[0] * r[0] + r[1] * r[1] + r[2] * r[2] for r in R]
    S = [[Fraction(sum(r[i] * r[j] for r in R), s2) for j in range(3)] for i in range(3)]
    g = [Fraction(sum(r[k] * q for r, q in zip(R, Q)), s3) for k in range(3)]
    sq = Fraction(sum(Q), s2)
    det = _det3(S)
    if det == 0:
        return dict(ok=True, params=None, singular=True)
    c = []
    for k in range(3):
        M = [[(g[i] if j == k else S[i][j]) for j in range(3)] for i in range(3)]
        c.append(_det3(M) / det / 2)
    r2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + sq / n
    return dict(ok=True, params=(mean[0] + c[0], mean[1] + c[1], mean[2] + c[2], _sqrt(r2)), singular=False)


def exact(kind, points):
    return exact_plane(points) if kind == PLANE else exact_sphere(points)


def err(params, exact_params) -> float:
    """max over the four parameters of |difference|, the difference taken exactly"""
    return float(max(abs(Fraction(float(p)) - e) for p, e in zip(params, exact_params)))


def err_mod_sign(params, exact_params) -> float:
    """err modulo the sign of (a, b, c, d): for plane cases whose branch the closed form does not decide"""
    return min(err(params, exact_params), err([-float(p) for p in params], exact_params))


def err_case(kind, params, ex) -> float:
    """err against the exact answer of a case; an undecided plane case (ex["gap"] < UNDECIDED_GAP) against the nearest of the
    branches rounding may take, modulo the sign of (a, b, c, d)"""
    if kind == PLANE and ex["gap"] < UNDECIDED_GAP:
        return min(err_mod_sign(params, alt) for alt in ex["alternatives"])
    return err(params, ex["params"])


def floor_F(inlier_points, exact_params) -> float:
    """F = 16 * 2^-53 * max(1, max |inlier coordinate|, max |exact parameter|): the rounding of the result itself, of the
    c0 + m addition and of the division by n"""
    m = max(1.0, float(np.abs(np.asarray(inlier_points)).max()), max(abs(float(e)) for e in exact_params))
    return 16.0 * 2.0 ** -53 * m


# ------------------------------------------------------------------------------------------------ fp64 emulations
# the closed forms of misc3d_amd/csrc/m3d_generalfit_fp.hpp in Python floats (IEEE doubles, every operation rounded once)
def moments_about_mean(mo, c0, n):
    mo = [float(v) for v in mo]
    n = float(n)
    m = [mo[0] / n, mo[1] / n, mo[2] / n]
    mean = [float(c0[k]) + m[k] for k in range(3)]
    S = mo[3:9]
    cen = [0.0] * 10
    cen[0] = S[0] - n * m[0] * m[0]
    cen[1] = S[1] - n * m[0] * m[1]
    cen[2] = S[2] - n * m[0] * m[2]
    cen[3] = S[3] - n * m[1] * m[1]
    cen[4] = S[4] - n * m[1] * m[2]
    cen[5] = S[5] - n * m[2] * m[2]
    trS = (S[0] + S[3]) + S[5]
    mm = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
    Sm = [(S[0] * m[0] + S[1] * m[1]) + S[2] * m[2], (S[1] * m[0] + S[3] * m[1]) + S[4] * m[2],
          (S[2] * m[0] + S[4] * m[1]) + S[5] * m[2]]
    f = 2.0 * n * mm - trS
    for k in range(3):
        cen[6 + k] = (mo[9 + k] - 2.0 * Sm[k]) + m[k] * f
    cen[9] = (cen[0] + cen[3]) + cen[5]
    return mean, cen


def plane_from_moments(mean, s):
    xx, xy, xz, yy, yz, zz = (float(v) for v in s[:6])
    det_x = yy * zz - yz * yz
    det_y = xx * zz - xz * xz
    det_z = xx * yy - xy * xy
    if det_x > det_y and det_x > det_z:
        a, b, c = det_x, xz * yz - xy * zz, xy * yz - xz * yy
    elif det_y > det_z:
        a, b, c = xz * yz - xy * zz, det_y, xy * xz - yz * xx
    else:
        a, b, c = xy * yz - xz * yy, xy * xz - yz * xx, det_z
    norm = float(np.sqrt((a * a + b * b) + c * c))
    if norm < 1.0e-8:
        return False, None
    a, b, c = a / norm, b / norm, c / norm
    return True, np.array([a, b, c, -((a * mean[0] + b * mean[1]) + c * mean[2])])


def sphere_from_moments(mean, s, n):
    s = [float(v) for v in s]
    A = [[4 * s[0], 4 * s[1], 4 * s[2], 2 * s[6]], [4 * s[1], 4 * s[3], 4 * s[4], 2 * s[7]],
         [4 * s[2], 4 * s[4], 4 * s[5], 2 * s[8]]]
    for col in range(3):
        piv = col
        for r in range(col + 1, 3):
            if abs(A[r][col]) > abs(A[piv][col]):
                piv = r
        A[piv], A[col] = A[col], A[piv]
        if A[col][col] == 0.0:
            continue
        for r in range(col + 1, 3):
            f = A[r][col] / A[col][col]
            for k in range(col, 4):
                A[r][k] -= f * A[col][k]
    c = [0.0] * 3
    for r in (2, 1, 0):
        acc = A[r][3]
        for k in range(r + 1, 3):
            acc -= A[r][k] * c[k]
        c[r] = acc / A[r][r] if A[r][r] != 0.0 else 0.0
    w3 = s[9] / float(n)
    return True, np.array([mean[0] + c[0], mean[1] + c[1], mean[2] + c[2],
                           float(np.sqrt(((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) + w3))])


def _closed_form(kind, mean, cen, n):
    return plane_from_moments(mean, cen) if kind == PLANE else sphere_from_moments(mean, cen, n)


def raw_moments(points, c0):
    """compact_count_k<KIND, true>'s twelve sums about c0 in fp64 (numpy's pairwise sums: the order is free)"""
    s = np.asarray(points, dtype=np.float64).reshape(-1, 3) - np.asarray(c0, dtype=np.float64)
    sx, sy, sz = s[:, 0], s[:, 1], s[:, 2]
    q = (sx * sx + sy * sy) + sz * sz
    return [float(v.sum()) for v in (sx, sy, sz, sx * sx, sx * sy, sx * sz, sy * sy, sy * sz, sz * sz, sx * q, sy * q, sz * q)]


def emulate_fused(points, c0, kind):
    """the fused path: raw moments about c0 -> moments_about_mean -> closed form.  -> (ok, params)"""
    n = len(points)
    mean, cen = moments_about_mean(raw_moments(points, c0), c0, n)
    return _closed_form(kind, mean, cen, n)


def centred_moments(points):
    """sum_xyz_k + sum_moments_k in fp64: the mean, then the ten moments of r = p - mean"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    mean = [float(p[:, k].sum()) / float(n) for k in range(3)]
    r0, r1, r2 = p[:, 0] - mean[0], p[:, 1] - mean[1], p[:, 2] - mean[2]
    q = (r0 * r0 + r1 * r1) + r2 * r2
    return mean, [float(v.sum()) for v in (r0 * r0, r0 * r1, r0 * r2, r1 * r1, r1 * r2, r2 * r2, r0 * q, r1 * q, r2 * q, q)]


def emulate_two_pass(points, kind):
    mean, cen = centred_moments(points)
    return _closed_form(kind, mean, cen, len(points))


def exact_raw_moments(points, c0):
    """the twelve raw moments about c0, each summed exactly and rounded ONCE (input of tests/cpp/test_generalfit_fp.cpp)"""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    X, D = _scaled_ints(np.concatenate([pts, np.asarray(c0, dtype=np.float64).reshape(1, 3)]))
    C = X.pop()
    s = [[p[k] - C[k] for k in range(3)] for p in X]
    q = [v[0] * v[0] + v[1] * v[1] + v[2] * v[2] for v in s]
    out = [Fraction(sum(v[k] for v in s), D) for k in range(3)]
    out += [Fraction(sum(v[i] * v[j] for v in s), D * D) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    out += [Fraction(sum(v[k] * w for v, w in zip(s, q)), D * D * D) for k in range(3)]
    return [float(v) for v in out]


def exact_centred_moments(points):
    """(mean, ten centred moments), each computed exactly and rounded once"""
    n, mean, R, sc = _centred(points)
    s2, s3 = sc * sc, sc * sc * sc
    Q = [r[0] * r[0] + r[1] * r[1] + r[2] * r[2] for r in R]
    cen = [Fraction(sum(r[i] * r[j] for r in R), s2) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    cen += [Fraction(sum(r[k] * q for r, q in zip(R, Q)), s3) for k in range(3)]
    cen.append(Fraction(sum(Q), s2))
    return [float(v) for v in mean], [float(v) for v in cen]


# ------------------------------------------------------------------------------------------------ input families
class Case:
    """One input: a cloud with outliers whose RANSAC fit at (thr, max_iter, prob, seed) selects the structure."""

    def __init__(self, name, kind, pts, thr, max_iter=1000, prob=0.9999, seed=11, tie=False, cap=False, structure=None,
                 model=None, ransac=True):
        self.name, self.kind, self.pts, self.thr = name, kind, np.ascontiguousarray(pts, dtype=np.float64), float(thr)
        self.max_iter, self.prob, self.seed, self.tie, self.cap = int(max_iter), float(prob), int(seed), tie, cap
        self.structure = structure      # indices of the structure's points, where the test wants to name them
        self.model = model              # the structure's true parameters, where RefineModel is run on them
        # False: no RANSAC fit can select the structure -- a cap 1e5 away: the minimal sphere's 4 x 4 determinants cancel by
        # (offset / extent)^3 > 2^53 and every hypothesis is noise (the oracle returns 0) -- so the inliers are those of
        # `model` and only the RefineModel route (Cloud.refine, the two-pass sums) reaches GeneralFit
        self.ransac = ransac

    def __repr__(self):
        return f"Case({self.name}, n={len(self.pts)})"


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _frame(normal):
    normal = _unit(normal)
    a = _unit(np.cross(normal, [1.0, 0.0, 0.0] if abs(normal[0]) < 0.9 else [0.0, 1.0, 0.0]))
    return normal, a, np.cross(normal, a)


def _mix(rng, structure, outliers):
    pts = np.concatenate([structure, outliers])
    return pts[rng.permutation(len(pts))]


_CAP_AXIS = (0.3, -0.5, 0.81)


def sphere_points(rng, n, centre, radius, half_angle_deg, sigma):
    """n points on the cap of half-angle `half_angle_deg` about _CAP_AXIS (180: the full sphere), radial noise sigma"""
    axis, a, b = _frame(_CAP_AXIS)
    cos_t = rng.uniform(np.cos(np.deg2rad(half_angle_deg)), 1.0, size=(n, 1))
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
    phi = rng.uniform(0.0, 2.0 * np.pi, size=(n, 1))
    d = cos_t * axis + sin_t * (np.cos(phi) * a + np.sin(phi) * b)
    return np.asarray(centre, dtype=np.float64) + (radius + rng.normal(0.0, sigma, size=(n, 1))) * d


def _sphere_family(name, radius, half_angle_deg, shift=0.0, scale=1.0, n_in=3000, n_out=3000):
    def make(seed, orc=None):
        rng = np.random.default_rng([seed, 101])
        centre = np.array([0.3, -0.2, 1.0]) * scale
        s = sphere_points(rng, n_in, centre, radius, half_angle_deg, 0.002 * scale)
        mid = s.mean(axis=0)
        half = max(3.0 * np.abs(s - mid).max(), 0.3 * scale)
        pts = _mix(rng, s, mid + rng.uniform(-half, half, size=(n_out, 3))) + shift
        return Case(name, SPHERE, pts, 0.01 * scale, seed=seed, cap=half_angle_deg < 90.0,
                    model=np.append(centre + shift, radius), ransac=shift < 1e5)
    return make


def plane_points(rng, n, normal, point, sigma, ext_u, ext_v):
    nrm, a, b = _frame(normal)
    u = rng.uniform(-ext_u, ext_u, size=(n, 1))
    v = rng.uniform(-ext_v, ext_v, size=(n, 1))
    return np.asarray(point, dtype=np.float64) + u * a + v * b + rng.normal(0.0, sigma, size=(n, 1)) * nrm


def _plane_family(name, ext_u, ext_v, shift=0.0, scale=1.0, n_in=3000, n_out=3000, box=None):
    def make(seed, orc=None):
        rng = np.random.default_rng([seed, 202])
        p0 = np.array([0.1, 0.2, -0.5]) * scale
        s = plane_points(rng, n_in, (0.2, -0.3, 0.93), p0, 0.002 * scale, ext_u * scale, ext_v * scale)
        half = (box if box is not None else 1.5 * max(ext_u, ext_v)) * scale
        pts = _mix(rng, s, p0 + rng.uniform(-half, half, size=(n_out, 3))) + shift
        return Case(name, PLANE, pts, 0.01 * scale, seed=seed)
    return make


def _plane_tie_family(name, sign):
    """normal (1, sign, 0) / sqrt 2: for every point (x, y, z) its mirror image -- (-y, -x, z) for sign +1, (y, x, z) for -1 --
    is in the cloud too, so the x and the y coordinates are the same multiset up to that sign and det_x == det_y EXACTLY:
    the closed form's first comparison is a tie that rounding decides.  (For sign -1 the two branches give opposite signs.)
    Noise and outliers are kept away from the threshold, so that the inliers are the structure, mirror images included."""
    def make(seed, orc=None):
        rng = np.random.default_rng([seed, 303])
        t = rng.uniform(-1.0, 1.0, size=1500)
        z = rng.uniform(-1.0, 1.0, size=1500) + 0.25
        e1, e2 = rng.uniform(-2e-4, 2e-4, size=(2, 1500))
        if sign > 0:    # plane x + y = 0
            half = np.stack([t + e1, -t + e2, z], axis=1)
            mirror = np.stack([-half[:, 1], -half[:, 0], half[:, 2]], axis=1)
        else:           # plane x - y = 0
            half = np.stack([t + e1, t + e2, z], axis=1)
            mirror = np.stack([half[:, 1], half[:, 0], half[:, 2]], axis=1)
        out = rng.uniform(-1.5, 1.5, size=(6000, 3))
        dist = np.abs(out[:, 0] + sign * out[:, 1]) / np.sqrt(2.0)
        out = out[dist > 0.1][:3000]
        return Case(name, PLANE, _mix(rng, np.concatenate([half, mirror]), out), 0.01, seed=seed, tie=True)
    return make


def _plane_cluster_family(name, extent):
    """a millimetre-scale (or smaller) planar cluster among far outliers: the closed form's `norm` is ~ (n extent^2 / 3)^2"""
    def make(seed, orc=None):
        rng = np.random.default_rng([seed, 404])
        p0 = np.array([0.1, 0.2, -0.5])
        s = plane_points(rng, 3000, (0.2, -0.3, 0.93), p0, extent / 500.0, extent, extent)
        return Case(name, PLANE, _mix(rng, s, p0 + rng.uniform(-1.0, 1.0, size=(1000, 3))), extent / 50.0, seed=seed)
    return make


def place(n, kind, seed, orc, anchors, rest, rest_index, outliers):
    """A cloud of n points whose hypothesis 0 (seed `seed`) samples `anchors`: the sample table depends on (n, seed) only
    (orc.draw_samples), so the anchors go where hypothesis 0 looks, `rest` at the free indices rest_index(free) picks, the
    outliers everywhere else.  -> (pts, indices of anchors + rest)"""
    m = 3 if kind == PLANE else 4
    sample = np.asarray(orc.draw_samples(n, m, 1, seed)[0], dtype=np.int64)
    assert len(anchors) == m and len(set(sample.tolist())) == m
    free = np.setdiff1d(np.arange(n, dtype=np.int64), sample)
    where = np.asarray(rest_index(free), dtype=np.int64)
    assert len(where) == len(rest) and len(outliers) == n - m - len(rest)
    pts = np.empty((n, 3))
    mask = np.zeros(n, dtype=bool)
    pts[sample], mask[sample] = anchors, True
    pts[where], mask[where] = rest, True
    pts[~mask] = outliers
    return pts, np.flatnonzero(mask)


def _tiny_family(name, kind, k):
    """exactly k inliers: k points of a structure (the first 3 resp. 4 where hypothesis 0 samples) among 60 scattered points,
    no four of which are coplanar / no five of which are cospherical within the threshold"""
    def make(seed, orc):
        rng = np.random.default_rng([seed, 505, k])
        m = 3 if kind == PLANE else 4
        if kind == PLANE:
            s = plane_points(rng, k, (0.2, -0.3, 0.93), (0.1, 0.2, -0.5), 1e-7, 1.0, 1.0)
        else:
            s = sphere_points(rng, k, (0.3, -0.2, 1.0), 0.5, 180.0, 1e-7)
        n = 60 + k
        out = rng.uniform(-10.0, 10.0, size=(60, 3))
        pts, idx = place(n, kind, seed, orc, s[:m], s[m:], lambda free: rng.choice(free, size=k - m, replace=False), out)
        return Case(name, kind, pts, 1e-5, max_iter=40, seed=seed, structure=idx)
    return make


SPHERE_FAMILIES = {
    "sphere_full": _sphere_family("sphere_full", 0.5, 180.0),
    "sphere_cap20": _sphere_family("sphere_cap20", 0.5, 20.0),
    "sphere_cap10": _sphere_family("sphere_cap10", 0.5, 10.0),
    "sphere_cap5_r5": _sphere_family("sphere_cap5_r5", 5.0, 5.0),
    "sphere_cap10_at_1e3": _sphere_family("sphere_cap10_at_1e3", 0.5, 10.0, shift=1e3),
    "sphere_cap10_at_1e5": _sphere_family("sphere_cap10_at_1e5", 0.5, 10.0, shift=1e5),
    "sphere_cap5_r5_at_1e3": _sphere_family("sphere_cap5_r5_at_1e3", 5.0, 5.0, shift=1e3),
    "sphere_cap5_r5_at_1e5": _sphere_family("sphere_cap5_r5_at_1e5", 5.0, 5.0, shift=1e5),
    "sphere_r1mm": _sphere_family("sphere_r1mm", 0.5e-3, 180.0, scale=1e-3),
    "sphere_4_inliers": _tiny_family("sphere_4_inliers", SPHERE, 4),
    "sphere_5_inliers": _tiny_family("sphere_5_inliers", SPHERE, 5),
    "sphere_6_inliers": _tiny_family("sphere_6_inliers", SPHERE, 6),
}
CAP_FAMILIES = [k for k in SPHERE_FAMILIES if "cap" in k]
PLANE_FAMILIES = {
    "plane_tilt": _plane_family("plane_tilt", 1.0, 1.0),
    "plane_tilt_at_1e4": _plane_family("plane_tilt_at_1e4", 1.0, 1.0, shift=1e4),
    "plane_tilt_at_1e6": _plane_family("plane_tilt_at_1e6", 1.0, 1.0, shift=1e6),
    "plane_strip_100x0.1": _plane_family("plane_strip_100x0.1", 50.0, 0.05, box=50.0),
    "plane_near_collinear": _plane_family("plane_near_collinear", 1.0, 0.003),
    "plane_tie_110": _plane_tie_family("plane_tie_110", +1),
    "plane_tie_1m10": _plane_tie_family("plane_tie_1m10", -1),
    "plane_3_inliers": _tiny_family("plane_3_inliers", PLANE, 3),
    "plane_4_inliers": _tiny_family("plane_4_inliers", PLANE, 4),
    "plane_cluster_norm_below": _plane_cluster_family("plane_cluster_norm_below", 1.0e-4),
    "plane_cluster_norm_above": _plane_cluster_family("plane_cluster_norm_above", 1.5e-3),
}
TIE_FAMILIES = ("plane_tie_110", "plane_tie_1m10")
FAIL_FAMILIES = ("plane_cluster_norm_below",)
FAMILIES = {**SPHERE_FAMILIES, **PLANE_FAMILIES}
FAMILY_SEED = 11


def family(name, orc=None, seed=FAMILY_SEED) -> Case:
    return FAMILIES[name](seed, orc)


# ---- seams: cloud sizes at kCompactTile and at the strides of the folds of its partials
K_TILE = 2048
SEAM_SIZES = (2047, 2048, 2049, 64 * 2048 - 1, 64 * 2048 + 1, 65 * 2048, 1024 * 2048 + 1)
SEAM_LAYOUTS = ("spread", "last_tile", "tile_0")
SEAM_INLIERS = 2000


def seam_structure(kind):
    """the structure every seam cloud carries: 3 resp. 4 noise-free anchors (hypothesis 0's sample: its minimal model is the
    true one to rounding, so every point of the structure is an inlier) and SEAM_INLIERS - m points with bounded noise.
    The SET of inliers is the same in every seam cloud, so one exact reference serves them all."""
    rng = np.random.default_rng([77, kind])
    m = 3 if kind == PLANE else 4
    k = SEAM_INLIERS - m
    if kind == PLANE:
        nrm, a, b = _frame((0.2, -0.3, 0.93))
        p0 = np.array([0.1, 0.2, -0.5])
        anchors = p0 + np.array([[0.9, -0.8], [-0.9, -0.7], [0.1, 0.95]]) @ np.stack([a, b])
        uv = rng.uniform(-1.0, 1.0, size=(k, 2))
        rest = p0 + uv @ np.stack([a, b]) + rng.uniform(-1e-3, 1e-3, size=(k, 1)) * nrm
    else:
        centre, radius, half = np.array([0.3, -0.2, 1.0]), 0.5, 20.0
        axis, a, b = _frame(_CAP_AXIS)
        st, ct = np.sin(np.deg2rad(half)), np.cos(np.deg2rad(half))
        dirs = [axis] + [ct * axis + st * (np.cos(p) * a + np.sin(p) * b) for p in (0.0, 2.1, 4.2)]
        anchors = centre + radius * np.array(dirs)
        s = sphere_points(rng, k, centre, radius, half, 0.0)
        rest = centre + (s - centre) * (1.0 + rng.uniform(-1e-3, 1e-3, size=(k, 1)))
    return anchors, rest


def seam_case(kind, n, layout, orc, seed=5) -> Case:
    anchors, rest = seam_structure(kind)
    k = len(rest)
    rng = np.random.default_rng([n, kind, SEAM_LAYOUTS.index(layout)])
    if layout == "spread":
        pick = lambda free: np.sort(rng.choice(free, size=k, replace=False))
    elif layout == "last_tile":
        pick = lambda free: free[-k:]
    else:
        pick = lambda free: free[:k]
    m = len(anchors)
    out = rng.uniform(50.0, 150.0, size=(n - m - k, 3))      # far from the structure and from one another
    pts, idx = place(n, kind, seed, orc, anchors, rest, pick, out)
    return Case(f"seam_{'plane' if kind == PLANE else 'sphere'}_{n}_{layout}", kind, pts, 0.01, max_iter=24, seed=seed,
                structure=idx)


def room(seed=3):
    """three planes of a room corner, 1700 + 1500 + 1300 points of 6000, for segment_plane_iterative"""
    rng = np.random.default_rng([seed, 606])
    walls = [plane_points(rng, 1700, (0.02, -0.01, 1.0), (0.0, 0.0, 0.0), 0.002, 1.0, 1.0),
             plane_points(rng, 1500, (1.0, 0.03, 0.02), (-1.0, 0.0, 1.0), 0.002, 1.0, 1.0),
             plane_points(rng, 1300, (-0.02, 1.0, 0.01), (0.0, -1.0, 1.0), 0.002, 1.0, 1.0)]
    n_out = 6000 - sum(len(w) for w in walls)
    return _mix(rng, np.concatenate(walls), rng.uniform(-1.0, 1.0, size=(n_out, 3)) + (0.0, 0.0, 1.0))


# ------------------------------------------------------------------------------------------------ the bound, shared work
# err(gpu) <= max(M err(oracle), F): M by measurement against the oracle's own error (tests/test_gpu_generalfit.py's header)
M_BOUND = 32.0
# the cap families on which the centre-based provisional centre of the sums is far enough outside the inliers for the loss
# to exceed M times the oracle's error; on the others (see test_generalfit.py) the two cannot be told apart by this bound
DISCRIMINATING_CAPS = ("sphere_cap10", "sphere_cap5_r5")


class Prepared:
    pass


_PREPARED = {}


def prepare(case_or_name, orc) -> Prepared:
    """Everything the tests of one input share, computed once per process and left unchanged: the case, the oracle's fit (or,
    where no RANSAC fit can select the structure, its RefineModel on the true model), the inlier points, the exact answer,
    F, the oracle's own error against the exact answer (None where the exact closed form fails) and the bound."""
    case = family(case_or_name, orc) if isinstance(case_or_name, str) else case_or_name
    if case.name in _PREPARED:
        return _PREPARED[case.name]
    p = Prepared()
    p.case = case
    if case.ransac:
        o = orc.fit(case.kind, case.pts, None, thr=case.thr, max_iter=case.max_iter, prob=case.prob, seed=case.seed, trace=True)
        p.fit, p.oracle_params, p.oracle_ok, p.inliers = o, o.params.copy(), o.general_fit_ok, o.inliers.astype(np.int64)
        p.minimal = o.trace["models"][o.best_index].copy() if o.best_index >= 0 else None
        p.sample = o.trace["samples"][o.best_index].astype(np.int64) if o.best_index >= 0 else None
    else:
        ok, params, idx = orc.refine(case.kind, case.pts, case.thr, case.model)
        p.fit, p.oracle_params, p.oracle_ok, p.inliers, p.minimal, p.sample = None, params, ok, idx.astype(np.int64), None, None
    p.points = np.ascontiguousarray(case.pts[p.inliers])
    p.exact = exact(case.kind, p.points)
    if p.exact["params"] is None:
        p.F = p.oracle_err = p.bound = None
    else:
        p.F = floor_F(p.points, p.exact["params"])
        p.oracle_err = err_case(case.kind, p.oracle_params, p.exact)
        p.bound = max(M_BOUND * p.oracle_err, p.F)
    _PREPARED[case.name] = p
    return p


def device_c0(p: Prepared):
    """the provisional centre minimal_fit_k leaves in slots 4..6 of the winner's record: the plane's first sample point, the
    centroid of the sphere's four (the same expression)"""
    q = p.case.pts[p.sample]
    if p.case.kind == PLANE:
        return q[0].copy()
    return ((q[0] + q[1]) + (q[2] + q[3])) * 0.25


def ratio(p: Prepared, params) -> float:
    """err(params) / max(err(oracle), F): what M is measured in"""
    return err_case(p.case.kind, params, p.exact) / max(p.oracle_err, p.F)
