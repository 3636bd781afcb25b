"""The plain-C restatement of the coloured ICP contract (tests/cpp/colored_icp_ref.c) built into a temporary directory and loaded
with ctypes, the multi-scale restatement on top of it (levels from tests/cpp/voxel_ref.c, colours included), an independent numpy
restatement, and the coloured clouds and cases both coloured-ICP test files use."""
import ctypes as C
import os
import subprocess

import numpy as np

import icp_ref_util as iu

HERE = os.path.dirname(os.path.abspath(__file__))

NO_COLORS = "TransformationEstimationForColoredICP requires colors for the source and the target PointCloud."
BAD_LAMBDA = "lambda_geometric must be in [0, 1]."
LAMBDA = 0.968

_f, _p = iu._f, iu._p


class ColoredRef:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "colored_icp_ref.so")
        if not os.path.exists(so):
            subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(HERE, "cpp", "colored_icp_ref.c"),
                            "-o", so, "-lm"], check=True)
        L = C.CDLL(so)
        L.colored_ref_gradient.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
        L.colored_ref_gradient.restype = C.c_int
        L.colored_ref_icp.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double,
                                      C.c_double, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int] + [C.c_void_p] * 7
        L.colored_ref_icp.restype = C.c_int
        self.L = L
        self.plain = iu.IcpRef(tmpdir)
        self.voxel = self.plain.voxel

    def gradient(self, dst, nrm, col, radius, max_nn=30):
        """-> (gradients (n, 3), list lengths (n,), AtA (n, 3, 3))"""
        dst, nrm, col = (_f(a).reshape(-1, 3) for a in (dst, nrm, col))
        n = len(dst)
        g, nn, ata = np.zeros((max(n, 1), 3)), np.zeros(max(n, 1), dtype=np.int32), np.zeros((max(n, 1), 3, 3))
        assert self.L.colored_ref_gradient(_p(dst), _p(nrm), _p(col), n, float(radius), int(max_nn), _p(g), _p(nn), _p(ata)) == 0
        return g[:n], nn[:n], ata[:n]

    def icp(self, src, src_col, dst, nrm, dst_col, max_dist, init=None, max_iteration=30, lam=LAMBDA, order=1, rel_fitness=1e-6,
            rel_rmse=1e-6):
        """-> dict(T, fitness, inlier_rmse, correspondences, iterations, converged, corr)"""
        src, sc, dst, nrm, dc = (_f(a).reshape(-1, 3) for a in (src, src_col, dst, nrm, dst_col))
        Ti = _f(init if init is not None else np.eye(4)).reshape(16).copy()
        T = np.zeros(16)
        fit, rm = C.c_double(0), C.c_double(0)
        cnt = C.c_uint64(0)
        it, conv = C.c_int(0), C.c_int(0)
        corr = np.full(max(len(src), 1), -1, dtype=np.int64)
        rc = self.L.colored_ref_icp(_p(src), _p(sc), len(src), _p(dst), _p(nrm), _p(dc), len(dst), float(max_dist), float(lam),
                                    _p(Ti), int(max_iteration), rel_fitness, rel_rmse, int(order), _p(T),
                                    C.cast(C.byref(fit), C.c_void_p), C.cast(C.byref(rm), C.c_void_p),
                                    C.cast(C.byref(cnt), C.c_void_p), C.cast(C.byref(it), C.c_void_p),
                                    C.cast(C.byref(conv), C.c_void_p), _p(corr))
        if rc != 0:
            raise RuntimeError({1: iu.INVALID_DISTANCE, 2: BAD_LAMBDA}.get(rc, "colored_icp_ref: out of memory"))
        return {"T": T.reshape(4, 4), "fitness": fit.value, "inlier_rmse": rm.value, "correspondences": cnt.value,
                "iterations": it.value, "converged": conv.value, "corr": corr[: len(src)]}

    def multi_scale(self, src, src_col, dst, nrm, dst_col, voxel_sizes, max_iters, max_dist, init=None, lam=LAMBDA, order=1):
        """MultiScaleICP with ColoredICP restated: per level both clouds through voxel_ref.c with their colours (the target with
        its normals), colored_ref_icp seeded with the previous pose, then the information matrix of the original clouds"""
        T = np.eye(4) if init is None else _f(init).reshape(4, 4)
        levels = []
        for v, it in zip(voxel_sizes, max_iters):
            s = self.voxel(src, v, colors=src_col)
            d = self.voxel(dst, v, normals=nrm, colors=dst_col)
            r = self.icp(s["points"], s["colors"], d["points"], d["normals"], d["colors"], max_dist, T, it, lam, order)
            r["n_src"], r["n_dst"] = len(s["points"]), len(d["points"])
            levels.append(r)
            T = r["T"]
        info, n_info = self.plain.information(src, dst, float(voxel_sizes[-1]) * 1.4, T)
        return {"T": T, "info": info, "n_info": n_info, "levels": levels}


# ---- the numpy restatement (brute-force searches, numpy's solvers): the independent cross-check of colored_icp_ref.c
def _intensity(c):
    return ((c[:, 0] + c[:, 1]) + c[:, 2]) / 3.0


def gradient_numpy(dst, nrm, col, radius, max_nn=30):
    """-> (gradients, condition numbers of AtA (inf where nn < 4))"""
    dst, nrm, col = (_f(a).reshape(-1, 3) for a in (dst, nrm, col))
    n = len(dst)
    I = _intensity(col)
    ok = np.isfinite(dst).all(axis=1)
    g, cond = np.zeros((n, 3)), np.full(n, np.inf)
    r2 = float(radius) * float(radius)
    for k in range(n):
        if not ok[k]:
            continue
        d = dst[k] - dst
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        d2 = np.where(ok, d2, np.inf)
        L = np.argsort(d2, kind="stable")[:max_nn]          # (stable: the lower index first on equal d2)
        L = L[d2[L] < r2]
        nn = len(L)
        if nn < 4:
            continue
        p = dst[L[1:]]
        s = ((p - dst[k]) * nrm[k]).sum(axis=1)
        A = np.vstack([p - s[:, None] * nrm[k] - dst[k], (nn - 1) * nrm[k]])
        b = np.append(I[L[1:]] - I[k], 0.0)
        AtA = A.T @ A
        with np.errstate(all="ignore"):
            cond[k] = np.linalg.cond(AtA) if np.isfinite(AtA).all() else np.inf
            try:
                g[k] = np.linalg.solve(AtA, A.T @ b)
            except np.linalg.LinAlgError:
                g[k] = np.nan
    return g, cond


def icp_numpy(src, src_col, dst, nrm, dst_col, max_dist, init=None, max_iteration=30, lam=LAMBDA):
    src, sc, dst, nrm, dc = (_f(a).reshape(-1, 3) for a in (src, src_col, dst, nrm, dst_col))
    T = np.eye(4) if init is None else _f(init).reshape(4, 4).copy()
    mov = src @ T[:3, :3].T + T[:3, 3] if not np.array_equal(T, np.eye(4)) else src.copy()
    r2 = float(max_dist) * float(max_dist)
    grad, _ = gradient_numpy(dst, nrm, dc, 2.0 * max_dist, 30)
    Is, It = _intensity(sc), _intensity(dc)
    sg, sp = np.sqrt(lam), np.sqrt(1.0 - lam)

    def result():
        corr, d2 = iu._nearest_numpy(mov, dst, r2)
        c = int((corr >= 0).sum())
        return corr, c, c / len(src), (np.sqrt(d2[corr >= 0].sum() / c) if c else 0.0)

    corr, cnt, fit, rm = result()
    it, conv = 0, 0
    while it < max_iteration:
        U = np.eye(4)
        m = corr >= 0
        if cnt:
            s, j = mov[m], corr[m]
            t, n, g = dst[j], nrm[j], grad[j]
            e = ((s - t) * n).sum(axis=1)
            q = s - e[:, None] * n - t
            I0 = (g * q).sum(axis=1) + It[j]
            mm = -(g - (g * n).sum(axis=1)[:, None] * n)
            J = np.vstack([sg * np.hstack([np.cross(s, n), n]), sp * np.hstack([np.cross(s, mm), mm])])
            r = np.concatenate([sg * e, sp * (Is[m] - I0)])
            A, b = J.T @ J, J.T @ r
            det = np.linalg.det(A)
            if np.isfinite(det) and abs(det) >= 1e-6:
                x = np.linalg.solve(A, -b)
                c, sn = np.cos(x[:3]), np.sin(x[:3])
                Rx = np.array([[1, 0, 0], [0, c[0], -sn[0]], [0, sn[0], c[0]]])
                Ry = np.array([[c[1], 0, sn[1]], [0, 1, 0], [-sn[1], 0, c[1]]])
                Rz = np.array([[c[2], -sn[2], 0], [sn[2], c[2], 0], [0, 0, 1]])
                U[:3, :3], U[:3, 3] = Rz @ Ry @ Rx, x[3:]
        T = U @ T
        mov = mov @ U[:3, :3].T + U[:3, 3]
        fit0, rm0 = fit, rm
        corr, cnt, fit, rm = result()
        it += 1
        if abs(fit0 - fit) < 1e-6 and abs(rm0 - rm) < 1e-6:
            conv = 1
            break
    return {"T": T, "fitness": fit, "inlier_rmse": rm, "correspondences": cnt, "iterations": it, "converged": conv, "corr": corr}


# ---- the clouds
def color_field(p):
    """a smooth colour field over space: sums of sines of position, other weights per channel, values in about [0.1, 0.9]"""
    p = np.nan_to_num(_f(p).reshape(-1, 3), nan=0.0, posinf=0.0, neginf=0.0)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    r = 0.5 + 0.20 * np.sin(5.0 * x + 1.0) + 0.15 * np.sin(4.0 * y - 2.0 * z)
    g = 0.5 + 0.18 * np.sin(6.0 * y + 0.5) + 0.12 * np.sin(3.0 * z + 4.0 * x)
    b = 0.5 + 0.22 * np.sin(4.5 * z - 1.0) + 0.10 * np.sin(5.0 * x - 3.0 * y)
    return np.ascontiguousarray(np.stack([r, g, b], axis=1))


def colors_of(c, seed=77, noise=0.002):
    """the colours of a case of icp_ref_util: the field on the source surface; the target carries the same field (read at the
    target points moved back by the case's true pose) plus small noise -> (src_colors, dst_colors)"""
    T = c.get("T", np.eye(4))
    back = (np.nan_to_num(c["dst"], nan=0.0, posinf=0.0, neginf=0.0) - T[:3, 3]) @ T[:3, :3]
    rng = np.random.default_rng(seed)
    return color_field(c["src"]), color_field(back) + rng.normal(0, noise, size=(len(c["dst"]), 3))


def case(name):
    """the coloured twin of iu.case(name): + src_colors, dst_colors"""
    c = iu.case(name)
    c["src_colors"], c["dst_colors"] = colors_of(c)
    return c


CASES = iu.CASES


def sized_case(n_src, max_iteration=3):
    """the coloured twin of iu.sized_case(n_src): the iteration kernel's seams"""
    c = iu.sized_case(n_src, max_iteration)
    c["src_colors"], c["dst_colors"] = colors_of(c)
    return c


def multi_case(n=20000):
    m = iu.multi_case(n)
    m["src_colors"], m["dst_colors"] = colors_of(m)
    return m


def slide_case(n=1500, seed=9, shift=(0.004, -0.003)):
    """"colour matters": one planar textured patch (z = 0, unit normal z), the target the same points permuted with a little
    in-plane noise (the final rmse is then a quantity, not the rounding of a zero), an in-plane offset as init.  Point-to-plane ICP cannot see the slide (its JTJ is singular: the update is the identity); the colours can."""
    rng = np.random.default_rng(seed)
    src = np.zeros((n, 3))
    src[:, :2] = rng.uniform(-0.3, 0.3, size=(n, 2))
    perm = rng.permutation(n)
    dst = np.ascontiguousarray(src[perm])
    dst[:, :2] += rng.normal(0, 0.0005, size=(n, 2))
    nrm = np.tile([0.0, 0.0, 1.0], (n, 1))

    def tex(p):
        x, y = p[:, 0], p[:, 1]
        r = 0.5 + 0.3 * np.sin(18.0 * x) * np.cos(7.0 * y)
        g = 0.5 + 0.3 * np.sin(15.0 * y + 1.0) * np.cos(5.0 * x)
        b = 0.5 + 0.3 * np.sin(11.0 * (x + y))
        return np.ascontiguousarray(np.stack([r, g, b], axis=1))
    init = np.eye(4)
    init[0, 3], init[1, 3] = shift
    return dict(src=src, dst=dst, dst_normals=nrm, src_colors=tex(src), dst_colors=tex(src[perm]), max_dist=0.03, init=init,
                max_iteration=30, T=np.eye(4), shift=np.array(shift))


def ramp_case(a=0.7, b=-0.4, c=0.3, h=0.1, m=9):
    """a regular m x m planar grid (spacing h, z = 0, normal z) with I = a x + b y + c, and three lone points far away (nn < 4)"""
    gx, gy = np.meshgrid(np.arange(m) * h, np.arange(m) * h, indexing="ij")
    pts = np.stack([gx.ravel(), gy.ravel(), np.zeros(m * m)], axis=1)
    pts = np.vstack([pts, [[50.0, 0, 0], [60.0, 0, 0], [60.0 + 0.5 * h, 0, 0]]])
    I = a * pts[:, 0] + b * pts[:, 1] + c
    interior = np.zeros(len(pts), dtype=bool)
    ij = np.stack([gx.ravel() / h, gy.ravel() / h], axis=1).round().astype(int)
    interior[: m * m] = ((ij >= 2) & (ij <= m - 3)).all(axis=1)
    return dict(points=np.ascontiguousarray(pts), normals=np.tile([0.0, 0.0, 1.0], (len(pts), 1)),
                colors=np.ascontiguousarray(np.stack([I, I, I], axis=1)), radius=2.5 * h, interior=interior,
                lone=np.arange(m * m, m * m + 3), gradient=np.array([a, b, 0.0]))


def seam_cloud(n, seed=0):
    """The gradient kernel's seams in one cloud of n >= 63 target points, radius 0.5, max_nn 30:
      [0, 40)  a jittered strip along x, spacing r / 15.2: list lengths 16 .. 30 cut by the radius (29 and 30 among them) and,
               in its middle, lists of more than 30 candidates cut by max_nn; row 5 has a zero normal
      40 .. 42 a cluster of 3 (nn = 3), 43 .. 46 a cluster of 4 (nn = 4)
      47       a point with a NaN coordinate (nn = 0), 48 a point with an infinite one
      49, 50   two points exactly the radius apart (d2 == r2: excluded, nn = 1 each)
      51, 52   copies of rows 38 and 39 (for the copy, L[0] is the original, not the point itself)
      53 .. 57 a cluster of 5 whose first row has a NaN colour (every gradient of the cluster is NaN)
      58 ..    sparse random points (lists cut by the radius)"""
    assert n >= 63
    rng = np.random.default_rng(100 + n + seed)
    r = 0.5
    d = r / 15.2
    pts = np.zeros((n, 3))
    pts[:40, 0] = np.arange(40) * d
    pts[:40, 1] = rng.uniform(-0.3, 0.3, 40) * d
    pts[:40, 2] = rng.uniform(-0.2, 0.2, 40) * d
    pts[40:43] = [10.0, 0, 0] + rng.uniform(-0.05, 0.05, (3, 3))
    pts[43:47] = [20.0, 0, 0] + rng.uniform(-0.05, 0.05, (4, 3))
    pts[47] = [np.nan, 1.0, 2.0]
    pts[48] = [30.0, np.inf, 0.0]
    pts[49], pts[50] = [64.0, 0, 0], [64.5, 0, 0]
    pts[51], pts[52] = pts[38], pts[39]
    pts[53:58] = [40.0, 0, 0] + rng.uniform(-0.05, 0.05, (5, 3))
    pts[58:] = [0.0, 5.0, 0.0] + rng.uniform(-1.0, 1.0, (n - 58, 3)) * [1.2, 1.2, 0.1]
    nrm = np.tile([0.0, 0.0, 1.0], (n, 1)) + rng.normal(0, 0.1, (n, 3))
    nrm[5] = 0.0
    col = color_field(pts * 3.0) + rng.normal(0, 0.01, (n, 3))
    col[53, 1] = np.nan
    return dict(points=np.ascontiguousarray(pts), normals=np.ascontiguousarray(nrm), colors=np.ascontiguousarray(col), radius=r,
                max_nn=30)
