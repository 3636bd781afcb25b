"""An independent reference for DetectBoundaryPoints and the inputs the boundary tests share.

The reference restates the CONTRACT, not the kernel: brute-force neighbourhoods ordered by (d2, index), the given normal
or the contract's covariance stand-in, and then the boundary decision in np.longdouble with a tangent basis of its own
(Gram-Schmidt from the coordinate axis least aligned with the normal) -- the largest angular gap does not depend on the
basis, only its roundings do.  compare() therefore leaves out the points whose gap lies within `margin` of the threshold;
every input family below is built so that there are none (tests/test_boundary.py asserts it).

margin = 1e-9 rad is derived, not measured: atan2 on either side is good to a few ulp of pi (~1e-15); two bases differ by
roundings of ~1e-16, amplified by at most 1 / conditioning, where conditioning = min over the neighbours of
|tangent projection| / |displacement|.  With conditioning >= 1e-6 (asserted per family) the total is <= 1e-10.
"""
import functools

import numpy as np

KNN, RADIUS, HYBRID = 0, 1, 2
LD = np.longdouble
MARGIN = 1e-9
MIN_CONDITIONING = 1e-6


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
class Ref:
    """per point: gap (rad; NaN where there is no decision to make), flag, cond, m (neighbours kept, self included),
    na (of those, the ones that do not coincide with the point); nb: the neighbour lists, (n, max m), padded with -1"""

    def __init__(self, gap, flag, cond, m, na, nb, thr_rad):
        self.gap, self.flag, self.cond, self.m, self.na, self.nb, self.thr_rad = gap, flag, cond, m, na, nb, thr_rad

    @property
    def indices(self):
        return np.flatnonzero(self.flag)


_nb_cache = {}


def neighbourhoods(pts, search, radius, max_nn):
    """-> (nb (n, mmax) int64 padded with -1, m (n,)): per point the neighbours (self included) ordered by (d2, index).
    Radius keeps d2 <= r*r, Hybrid the max_nn smallest of d2 < r*r, KNN the max_nn smallest.  A point with a non-finite
    coordinate has no neighbours and is nobody's neighbour."""
    pts = np.ascontiguousarray(pts, np.float64)
    key = (pts.tobytes(), pts.shape, search, float(radius), int(max_nn))
    if key in _nb_cache:
        return _nb_cache[key]
    n = len(pts)
    fin = np.isfinite(pts).all(axis=1)
    cand = np.flatnonzero(fin)
    P = pts[cand]
    r2 = float(radius) * float(radius)
    lists = [np.zeros(0, np.int64)] * n
    for i in cand:
        dx, dy, dz = pts[i, 0] - P[:, 0], pts[i, 1] - P[:, 1], pts[i, 2] - P[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        if search == RADIUS:
            sel = np.flatnonzero(d2 <= r2)
        elif search == HYBRID:
            sel = np.flatnonzero(d2 < r2)
        else:
            sel = np.arange(len(P))
        if search != RADIUS and len(sel) > max_nn:          # everything up to the max_nn-th distance, ties included
            sel = sel[d2[sel] <= np.partition(d2[sel], max_nn - 1)[max_nn - 1]]
        order = np.lexsort((cand[sel], d2[sel]))
        if search != RADIUS:
            order = order[:max_nn]
        lists[i] = cand[sel[order]]
    m = np.array([len(l) for l in lists], np.int64)
    nb = np.full((n, max(int(m.max()) if n else 0, 1)), -1, np.int64)
    for i, l in enumerate(lists):
        nb[i, :len(l)] = l
    _nb_cache[key] = (nb, m)
    return nb, m


def standin_normals(pts, nb, m, eigvec):
    """the contract's stand-in for a missing normal: nine cumulants summed sequentially in neighbour order (np.cumsum
    is sequential), times 1/m, C = E[x x^T] - E[x] E[x]^T, smallest eigenvector through `eigvec` (oracle.j3x3_...)"""
    n = len(pts)
    out = np.full((n, 3), np.nan)
    valid = nb >= 0
    q = np.where(valid[..., None], pts[np.where(valid, nb, 0)], 0.0)        # (n, mmax, 3); the padding adds +0.0
    x, y, z = q[..., 0], q[..., 1], q[..., 2]
    terms = np.stack([x, y, z, x * x, x * y, x * z, y * y, y * z, z * z], -1)
    cs = np.cumsum(terms, axis=1)
    for i in np.flatnonzero(m >= 3):
        s = cs[i, m[i] - 1] * (1.0 / float(m[i]))
        C = np.empty(9)
        C[0] = s[3] - s[0] * s[0]
        C[1] = s[4] - s[0] * s[1]
        C[2] = s[5] - s[0] * s[2]
        C[4] = s[6] - s[1] * s[1]
        C[5] = s[7] - s[1] * s[2]
        C[8] = s[8] - s[2] * s[2]
        C[3], C[6], C[7] = C[1], C[2], C[5]
        out[i] = eigvec(C)
    return out


def decide(pts, normals, nb, m, thr_deg):
    """the boundary decision in np.longdouble, with a basis of its own -> Ref"""
    n = len(pts)
    thr = float(LD(thr_deg) * LD(np.pi) / LD(180))
    gap = np.full(n, np.nan)
    cond = np.full(n, np.inf)
    na = np.zeros(n, np.int64)
    flag = np.zeros(n, bool)
    for i in np.flatnonzero(m >= 3):
        nrm = normals[i].astype(LD)
        d = pts[nb[i, :m[i]]].astype(LD) - pts[i].astype(LD)
        d = d[(d != 0).any(axis=1)]                          # coincident neighbours (the point itself among them)
        na[i] = len(d)
        n64 = normals[i]
        with np.errstate(over="ignore", invalid="ignore"):    # the contract measures the normal's length in double
            l64 = np.sqrt((n64[0] * n64[0] + n64[1] * n64[1]) + n64[2] * n64[2])
        if len(d) == 0 or not (l64 > 0 and np.isfinite(l64)):  # nothing to measure, or no direction to measure against:
            continue                                            # never flagged, whatever the threshold
        nrm = nrm / np.sqrt((nrm * nrm).sum())
        e = np.zeros(3, LD)
        e[np.argmin(np.abs(nrm))] = 1
        u = e - (e @ nrm) * nrm
        u = u / np.sqrt((u * u).sum())
        v = np.cross(nrm, u)
        a, b = d @ u, d @ v
        cond[i] = float((np.sqrt(a * a + b * b) / np.sqrt((d * d).sum(axis=1))).min())
        ang = np.sort(np.arctan2(b, a))
        g = 2 * LD(np.pi) - ang[-1] + ang[0]
        if len(ang) > 1:
            g = max(g, np.diff(ang).max())
        gap[i] = float(g)
        flag[i] = g > LD(thr_deg) * LD(np.pi) / LD(180)
    return Ref(gap, flag, cond, m, na, nb, thr)


def reference(pts, normals, search, radius, max_nn, thr_deg, eigvec):
    """pts (n, 3), normals (n, 3) or None, eigvec: oracle.j3x3_smallest_eigvec -> Ref"""
    pts = np.ascontiguousarray(pts, np.float64)
    nb, m = neighbourhoods(pts, search, radius, max_nn)
    nrm = np.asarray(normals, np.float64) if normals is not None else standin_normals(pts, nb, m, eigvec)
    return decide(pts, nrm, nb, m, thr_deg)


def compare(flags_under_test, ref, margin=MARGIN):
    """flags_under_test: a bool array over the points, or the array of flagged indices.  Points whose gap is within
    `margin` of the threshold are undecided and left out; everywhere else the flags must be equal.  -> number left out"""
    f = np.asarray(flags_under_test)
    if f.dtype != bool:
        idx = f.astype(np.int64)
        f = np.zeros(len(ref.flag), bool)
        f[idx] = True
    undecided = np.abs(ref.gap - ref.thr_rad) < margin      # NaN gaps (no decision: never flagged) compare False
    bad = np.flatnonzero((f != ref.flag) & ~undecided)
    assert len(bad) == 0, (f"{len(bad)} points differ from the reference, first {bad[:8].tolist()}: "
                           f"flag under test {f[bad[:8]].tolist()}, gap {np.degrees(ref.gap[bad[:8]]).tolist()} deg, "
                           f"threshold {np.degrees(ref.thr_rad)} deg, m {ref.m[bad[:8]].tolist()}")
    return int(undecided.sum())


# ------------------------------------------------------------------------------------------------
# input families (every cloud is in random order: the original index is never the grid order)
# ------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


SHELL_CUT = 0.6                                                     # the cap z > 0.6 is cut off the unit sphere


@functools.lru_cache(None)
def shell(n=3000, seed=11):
    """unit sphere without the cap z > SHELL_CUT, analytic normals: every octant, every branch of the tangent basis"""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(4 * n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    p = p[p[:, 2] < SHELL_CUT][:n]
    assert len(p) == n
    return np.ascontiguousarray(p * (1 + rng.normal(0, 1e-4, (n, 1)))), np.ascontiguousarray(p)


def rim_distance(p):
    """arc distance on the unit sphere from p's direction to the rim of the cut"""
    return np.abs(np.arccos(np.clip(p[:, 2] / np.linalg.norm(p, axis=1), -1, 1)) - np.arccos(SHELL_CUT))


def plane_patch(normal, n=600, seed=5, offset=(0.0, 0.0, 0.0), noise=1e-4):
    """a unit square patch through `offset` orthogonal to `normal`, with a disc cut out of it"""
    rng = np.random.default_rng(seed)
    nrm = _unit(normal)
    a = np.zeros(3)
    a[np.argmin(np.abs(nrm))] = 1
    a = _unit(a - (a @ nrm) * nrm)
    b = np.cross(nrm, a)
    uv = rng.uniform(0, 1, (2 * n, 2))
    uv = uv[np.hypot(uv[:, 0] - 0.5, uv[:, 1] - 0.5) > 0.18][:n]
    p = uv[:, :1] * a + uv[:, 1:] * b + rng.normal(0, noise, (len(uv), 1)) * nrm + np.asarray(offset, np.float64)
    return np.ascontiguousarray(p), np.tile(np.asarray(normal, np.float64), (len(p), 1))


AXIS_NORMALS = {"+x": (1, 0, 0), "-x": (-1, 0, 0), "+y": (0, 1, 0), "-y": (0, -1, 0), "+z": (0, 0, 1), "-z": (0, 0, -1),
                "xy": tuple(np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)), "xyz": tuple(np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0))}

SEAM_RADIUS = 3.08


@functools.lru_cache(None)
def seam_cloud():
    """a jittered 28 x 28 lattice in a tilted plane: every point has at most 32 points strictly inside SEAM_RADIUS, most
    of the interior close to that many, and no d2 equals the squared radius"""
    rng = np.random.default_rng(21)
    g = np.stack(np.meshgrid(np.arange(28.0), np.arange(28.0), indexing="ij"), -1).reshape(-1, 2)
    g = g + rng.uniform(-0.1, 0.1, g.shape)
    nrm = _unit([0.3, -0.5, 0.8])
    a = _unit(np.cross(nrm, [0, 0, 1.0]))
    b = np.cross(nrm, a)
    p = g[:, :1] * a + g[:, 1:] * b + rng.normal(0, 1e-3, (len(g), 1)) * nrm
    p = p[rng.permutation(len(p))]
    return np.ascontiguousarray(p), np.tile(nrm, (len(p), 1))


RADIUS_CAP_R = 1.0


@functools.lru_cache(None)
def radius_cap_cloud(in_ball=128):
    """`in_ball` points inside a ball of diameter 0.8 < r = 1 (each of them has exactly `in_ball` neighbours) and a sparse
    planar remainder far from it"""
    rng = np.random.default_rng(31)
    ball = rng.normal(size=(in_ball, 3))
    ball *= (0.4 * rng.uniform(0, 1, (in_ball, 1)) ** (1 / 3)) / np.linalg.norm(ball, axis=1, keepdims=True)
    rest = np.c_[rng.uniform(5, 15, (300, 2)), rng.normal(0, 1e-3, 300)]
    p = np.r_[ball, rest]
    return np.ascontiguousarray(p[rng.permutation(len(p))])


@functools.lru_cache(None)
def tie_lattice(side=30):
    """integer lattice in z = 0, normals e_z, shuffled: every d2 is exact and most of them tie"""
    g = np.stack(np.meshgrid(np.arange(float(side)), np.arange(float(side)), indexing="ij"), -1).reshape(-1, 2)
    p = np.c_[g, np.zeros(len(g))]
    p = p[np.random.default_rng(41).permutation(len(p))]
    return np.ascontiguousarray(p), np.tile([0.0, 0.0, 1.0], (len(p), 1))


@functools.lru_cache(None)
def duplicates_cloud():
    """a patch with one point repeated 40 times and scattered pairs and triples"""
    p, nrm = plane_patch((-0.3, 0.2, 1.0), n=500, seed=51)
    rng = np.random.default_rng(52)
    p = np.r_[p, np.tile(p[17], (39, 1)), p[[40, 41, 42, 43, 44]], p[[40, 41]]]     # 17: x40; 40, 41: x3; 42..44: x2
    perm = rng.permutation(len(p))
    return np.ascontiguousarray(p[perm]), np.tile(nrm[0], (len(p), 1))


@functools.lru_cache(None)
def nonfinite_shell():
    """1000 shell points, about 1 % of them with NaN, +Inf or -Inf in one or in all coordinates"""
    p, nrm = shell(1000, seed=61)
    p, nrm = p.copy(), nrm.copy()
    bad = [np.nan, np.inf, -np.inf]
    for t, i in enumerate(range(7, 1000, 83)):               # 12 points
        if t % 4 == 3:
            p[i] = bad[t % 3]
        else:
            p[i, t % 3] = bad[(t // 3) % 3]
    return p, nrm


def few_finite(k):
    """10 points of which exactly k are finite"""
    rng = np.random.default_rng(70 + k)
    p = rng.uniform(0, 1, (10, 3))
    kill = rng.permutation(10)[: 10 - k]
    for t, i in enumerate(kill):
        p[i, t % 3] = [np.nan, np.inf, -np.inf][t % 3]
    return p


def blob(n, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).normal(size=(n, 3)))


@functools.lru_cache(None)
def collinear(diagonal):
    t = np.random.default_rng(81).permutation(200) * 0.125 + 0.25        # exact in binary, distinct, shuffled
    p = np.c_[t, t, t] if diagonal else np.c_[t, np.zeros(200), np.zeros(200)]
    nrm = _unit([1, -1, 0]) if diagonal else np.array([0.0, 0.0, 1.0])
    return np.ascontiguousarray(p), np.tile(nrm, (200, 1))


@functools.lru_cache(None)
def two_clusters():
    """two tight clusters whose separation is 1000 times their size: the KNN walk crosses empty shells of cells"""
    rng = np.random.default_rng(91)
    a = rng.normal(0, 1e-3, (200, 3))
    b = rng.normal(0, 1e-3, (200, 3)) + np.array([3.0, 2.0, 1.0])
    p = np.r_[a, b]
    return np.ascontiguousarray(p[rng.permutation(400)])


@functools.lru_cache(None)
def outlier_cloud():
    p, nrm = plane_patch((-0.3, 0.2, 1.0), n=500, seed=95)
    p = np.r_[p, [[700.0, -400.0, 9000.0]]]
    perm = np.random.default_rng(96).permutation(len(p))
    return np.ascontiguousarray(p[perm]), np.tile(nrm[0], (len(p), 1))


def far_patch():
    """a flat patch 1e6 from the origin on every axis"""
    return plane_patch((-0.3, 0.2, 1.0), seed=97, offset=(1e6, 1e6, 1e6))


class Case:
    """one input: cloud, normals (or None), search parameters, threshold; oracle: whether the C oracle is defined on it
    (its KNN branch sorts NaN keys: not on non-finite points)"""

    def __init__(self, pts, nrm, search, radius, max_nn, thr=90.0, oracle=True):
        self.pts, self.nrm, self.search, self.radius, self.max_nn, self.thr, self.oracle = (
            np.ascontiguousarray(pts, np.float64), None if nrm is None else np.ascontiguousarray(nrm, np.float64), search,
            radius, max_nn, thr, oracle)

    def args(self):
        return self.pts, self.nrm, self.search, self.radius, self.max_nn, self.thr

    def reference(self, eigvec):
        return reference(self.pts, self.nrm, self.search, self.radius, self.max_nn, self.thr, eigvec)


# maps that move z: d2 = (dx^2 + dy^2) + dz^2 changes its association, so these are inputs of their own
Z_MAPS = {"zxy": lambda a: np.ascontiguousarray(a[:, [2, 0, 1]]), "swap_xz": lambda a: np.ascontiguousarray(a[:, [2, 1, 0]])}


def _build_cases():
    c = {}
    # all directions
    sp, sn = shell()
    c["shell-hybrid"] = lambda: Case(sp, sn, HYBRID, 0.2, 30)
    c["shell-knn"] = lambda: Case(sp, sn, KNN, 0.0, 30)
    c["shell-radius"] = lambda: Case(sp, sn, RADIUS, 0.15, 0)
    c["shell-estimated"] = lambda: Case(sp, None, HYBRID, 0.2, 30)
    c["shell-normals-x0.5"] = lambda: Case(sp, 0.5 * sn, HYBRID, 0.2, 30)
    c["shell-normals-x3"] = lambda: Case(sp, 3.0 * sn, HYBRID, 0.2, 30)
    c["shell-normals-negated"] = lambda: Case(sp, -sn, HYBRID, 0.2, 30)
    for name, f in Z_MAPS.items():
        c[f"shell-map-{name}"] = lambda f=f: Case(f(sp), f(sn), HYBRID, 0.2, 30)
    for name, nv in AXIS_NORMALS.items():
        c[f"patch-normal{name}"] = lambda nv=nv: Case(*plane_patch(nv), HYBRID, 0.12, 30)

    def bad_normals():
        p, nrm = shell(800, seed=13)
        nrm = nrm.copy()
        nrm[[3, 200]] = 0.0
        nrm[[4, 300]] = np.nan
        nrm[5, 1] = np.nan
        nrm[[6, 400], 0] = np.nan
        return Case(p, nrm, HYBRID, 0.35, 30)
    c["shell-zero-and-nan-normals"] = bad_normals

    def bad_normals_negative_threshold():                    # no direction: not flagged even where every gap passes
        case = bad_normals()
        nrm = case.nrm.copy()
        nrm[7], nrm[8, 2] = 1e200, np.inf                    # a length that overflows in double, an infinite one
        return Case(case.pts, nrm, HYBRID, 0.35, 30, -10.0)
    c["shell-zero-and-nan-normals-threshold--10"] = bad_normals_negative_threshold
    # LDS | scratch seam
    for search, sname in ((KNN, "knn"), (HYBRID, "hybrid")):
        for k in (1, 2, 3, 4, 31, 32, 33):
            for wn in (True, False):
                c[f"seam-{sname}-{k}-{'normals' if wn else 'estimated'}"] = lambda search=search, k=k, wn=wn: Case(
                    seam_cloud()[0], seam_cloud()[1] if wn else None, search, SEAM_RADIUS, k)
    c["seam-radius"] = lambda: Case(*seam_cloud(), RADIUS, SEAM_RADIUS, 0)
    # Radius cap
    c["radius-cap-128"] = lambda: Case(radius_cap_cloud(128), None, RADIUS, RADIUS_CAP_R, 0)
    # ties
    for thr in (100.0, 200.0):
        c[f"ties-radius-{thr:.0f}"] = lambda thr=thr: Case(*tie_lattice(), RADIUS, 2.0, 0, thr)
        c[f"ties-hybrid-all-{thr:.0f}"] = lambda thr=thr: Case(*tie_lattice(), HYBRID, 2.0, 64, thr)
        # the ring at d2 = 4 repeats the directions of the ring at d2 = 1, so it cannot change a gap; at radius 1 the ring ON
        # the radius is all there is: Radius sees gaps of 90 / 180 / 270 degrees, Hybrid fewer than 3 neighbours
        c[f"ties-radius-unit-{thr:.0f}"] = lambda thr=thr: Case(*tie_lattice(), RADIUS, 1.0, 0, thr)
        c[f"ties-hybrid-unit-{thr:.0f}"] = lambda thr=thr: Case(*tie_lattice(), HYBRID, 1.0, 30, thr)
        for k in (3, 4, 5, 6, 9):
            c[f"ties-knn-{k}-{thr:.0f}"] = lambda thr=thr, k=k: Case(*tie_lattice(), KNN, 0.0, k, thr)
            c[f"ties-hybrid-{k}-{thr:.0f}"] = lambda thr=thr, k=k: Case(*tie_lattice(), HYBRID, 3.5, k, thr)
    # duplicates
    for wn in (True, False):
        tag = "normals" if wn else "estimated"
        c[f"duplicates-hybrid-{tag}"] = lambda wn=wn: Case(duplicates_cloud()[0], duplicates_cloud()[1] if wn else None,
                                                          HYBRID, 0.15, 30)
        c[f"duplicates-knn-{tag}"] = lambda wn=wn: Case(duplicates_cloud()[0], duplicates_cloud()[1] if wn else None,
                                                       KNN, 0.0, 30)
    # non-finite points
    for search, sname, r, k in ((KNN, "knn", 0.0, 20), (RADIUS, "radius", 0.25, 0), (HYBRID, "hybrid", 0.3, 20)):
        for wn in (True, False):
            c[f"nonfinite-{sname}-{'normals' if wn else 'estimated'}"] = lambda search=search, r=r, k=k, wn=wn: Case(
                nonfinite_shell()[0], nonfinite_shell()[1] if wn else None, search, r, k, oracle=search != KNN)
    for k in (1, 2, 3):
        c[f"finite-{k}-of-10-knn"] = lambda k=k: Case(few_finite(k), None, KNN, 0.0, 5, oracle=False)
        c[f"finite-{k}-of-10-hybrid"] = lambda k=k: Case(few_finite(k), None, HYBRID, 10.0, 5)
        c[f"finite-{k}-of-10-radius"] = lambda k=k: Case(few_finite(k), None, RADIUS, 10.0, 0)
    # KNN walk
    for n in (1, 2, 3, 63, 64, 65, 129):
        c[f"walk-n{n}"] = lambda n=n: Case(blob(n, 100 + n), None, KNN, 0.0, 10)
    for diag in (False, True):
        for wn in (True, False):
            c[f"walk-collinear-{'diagonal' if diag else 'x'}-{'normals' if wn else 'estimated'}"] = lambda diag=diag, wn=wn: Case(
                collinear(diag)[0], collinear(diag)[1] if wn else None, KNN, 0.0, 10)
    c["walk-identical"] = lambda: Case(np.tile([0.3, -1.5, 2.0], (100, 1)), None, KNN, 0.0, 10)
    c["walk-two-clusters"] = lambda: Case(two_clusters(), None, KNN, 0.0, 50)
    for wn in (True, False):
        tag = "normals" if wn else "estimated"
        c[f"walk-outlier-{tag}"] = lambda wn=wn: Case(outlier_cloud()[0], outlier_cloud()[1] if wn else None, KNN, 0.0, 20)
        c[f"walk-offset-1e6-knn-{tag}"] = lambda wn=wn: Case(far_patch()[0], far_patch()[1] if wn else None, KNN, 0.0, 20)
    c["walk-offset-1e6-hybrid"] = lambda: Case(*far_patch(), HYBRID, 0.12, 30)
    # thresholds
    for thr in (0.0, -10.0, 361.0):
        c[f"threshold-{thr:.0f}"] = lambda thr=thr: Case(*duplicates_cloud(), HYBRID, 0.15, 30, thr)
    return c


CASES = _build_cases()
