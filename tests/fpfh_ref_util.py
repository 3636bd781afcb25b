"""The plain-C restatement of the fragment-preprocessing contract (tests/cpp/fpfh_ref.c: neighbourhood, normals, FPFH) built
into a temporary directory and loaded with ctypes, a vectorised numpy / scipy version of the same contract (the second
opinion on the C text), and the clouds the FPFH tests share."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KNN, RADIUS, HYBRID = 0, 1, 2


def build_ref(tmpdir):
    so = os.path.join(str(tmpdir), "fpfh_ref.so")
    if not os.path.exists(so):
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fopenmp", "-shared", "-fPIC",
                        os.path.join(HERE, "cpp", "fpfh_ref.c"), "-o", so, "-lm"], check=True)
    L = C.CDLL(so)
    P = C.c_void_p
    L.fpfh_ref_neighbours.argtypes = [P, C.c_size_t, C.c_int, C.c_double, C.c_int, P, P, P]
    L.fpfh_ref_pair_bins.argtypes = [P, C.c_size_t, P, P]
    L.fpfh_ref_compute.argtypes = [P, P, C.c_size_t, C.c_int, C.c_double, C.c_int, P, P]
    L.fpfh_ref_normals.argtypes = [P, C.c_size_t, C.c_int, C.c_double, C.c_int, C.c_int, P, P]
    for f in (L.fpfh_ref_neighbours, L.fpfh_ref_pair_bins, L.fpfh_ref_compute, L.fpfh_ref_normals):
        f.restype = None
    return Ref(L)


def _f(a):
    return np.ascontiguousarray(a, np.float64)


class Ref:
    def __init__(self, L):
        self.L = L

    def neighbours(self, xyz, search, radius, max_nn):
        """-> (idx int64 (n, max_nn) padded -1, d2 padded +inf, m int32 (n,))"""
        xyz = _f(xyz).reshape(-1, 3)
        n = len(xyz)
        idx = np.zeros((n, max_nn), np.int64)
        d2 = np.zeros((n, max_nn))
        cnt = np.zeros(n, np.int32)
        self.L.fpfh_ref_neighbours(xyz.ctypes.data, n, search, float(radius), max_nn, idx.ctypes.data, d2.ctypes.data,
                                   cnt.ctypes.data)
        return idx, d2, cnt

    def pair_bins(self, pairs):
        pairs = _f(pairs).reshape(-1, 12)
        bins = np.zeros((len(pairs), 3), np.int32)
        feat = np.zeros((len(pairs), 3))
        self.L.fpfh_ref_pair_bins(pairs.ctypes.data, len(pairs), bins.ctypes.data, feat.ctypes.data)
        return bins, feat

    def fpfh(self, xyz, normals, search, radius, max_nn, spfh=False):
        """-> (n, 33) rows (and the SPFH rows)"""
        xyz, normals = _f(xyz).reshape(-1, 3), _f(normals).reshape(-1, 3)
        n = len(xyz)
        out = np.zeros((n, 33))
        sp = np.zeros((n, 33))
        self.L.fpfh_ref_compute(xyz.ctypes.data, normals.ctypes.data, n, search, float(radius), max_nn, out.ctypes.data,
                                sp.ctypes.data)
        return (out, sp) if spfh else out

    def normals(self, xyz, search, radius, max_nn, orient_to=None):
        xyz = _f(xyz).reshape(-1, 3)
        cam = _f(orient_to if orient_to is not None else (0, 0, 0)).reshape(3)
        out = np.zeros((len(xyz), 3))
        self.L.fpfh_ref_normals(xyz.ctypes.data, len(xyz), search, float(radius), max_nn, int(orient_to is not None),
                                cam.ctypes.data, out.ctypes.data)
        return out

    def preprocess(self, xyz, voxel, normals=None):
        """PreProcessFragments by the contract: (normals, (n, 33) rows)"""
        xyz = _f(xyz).reshape(-1, 3)
        if normals is None:
            nrm = self.normals(xyz, HYBRID, 2.0 * voxel, 30, orient_to=(0, 0, 0))
        else:
            nrm = orient(xyz, _f(normals).reshape(-1, 3), (0, 0, 0))
        return nrm, self.fpfh(xyz, nrm, HYBRID, 5.0 * voxel, 100)


def orient(xyz, normals, cam):
    """OrientNormalsTowardsCameraLocation by the contract"""
    v = np.asarray(cam, np.float64)[None, :] - xyz
    out = normals.copy()
    zero = (out == 0).all(1)
    ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        out[zero] = np.where(ln[zero, None] == 0, np.array([0.0, 0.0, 1.0]), v[zero] / ln[zero, None])
    dotp = (out[:, 0] * v[:, 0] + out[:, 1] * v[:, 1]) + out[:, 2] * v[:, 2]
    flip = ~zero & (dotp < 0)
    out[flip] = -out[flip]
    return out


# ---- the numpy / scipy sketch of the same contract (finite clouds; self is entry 0 unless duplicated) ----------------------
def np_neighbours(pts, search, radius, max_nn):
    from scipy.spatial import cKDTree
    n = len(pts)
    k = min(max_nn + 8, n)   # (a few spare candidates: the tree's own rounding may order near-ties differently)
    t = cKDTree(pts)
    _, i = t.query(pts, k=k)
    i = i.reshape(n, k)
    dx = pts[:, None, :] - pts[i]
    d2 = (dx[..., 0] * dx[..., 0] + dx[..., 1] * dx[..., 1]) + dx[..., 2] * dx[..., 2]
    order = np.lexsort((i, d2), axis=1)
    i = np.take_along_axis(i, order, 1)[:, :max_nn]
    d2 = np.take_along_axis(d2, order, 1)[:, :max_nn]
    valid = np.isfinite(d2)
    if search == HYBRID:
        valid &= d2 < radius * radius
    return i, d2, valid


def np_pair_bins(p1, n1, p2, n2):
    dp = p2 - p1
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    d = np.sqrt(dot(dp, dp))
    zero = d == 0
    ds = np.where(zero, 1, d)
    a1 = dot(n1, dp) / ds
    a2 = dot(n2, dp) / ds
    sw = np.arccos(np.abs(a1)) > np.arccos(np.abs(a2))
    m = sw[..., None]
    na = np.where(m, n2, n1)
    nb = np.where(m, n1, n2)
    dp = np.where(m, -dp, dp)
    f2 = np.where(sw, -a2, a1)
    v = np.cross(dp, na)
    vn = np.sqrt(dot(v, v))
    zero = zero | (vn == 0)
    v = v / np.where(vn == 0, 1, vn)[..., None]
    w = np.cross(na, v)
    f1 = dot(v, nb)
    f0 = np.arctan2(dot(w, nb), dot(na, nb))
    f0, f1, f2 = (np.where(zero, 0.0, f) for f in (f0, f1, f2))
    b0 = np.clip(np.floor(11 * (f0 + np.pi) / (2 * np.pi)), 0, 10).astype(np.int64)
    b1 = np.clip(np.floor(11 * (f1 + 1) * 0.5), 0, 10).astype(np.int64)
    b2 = np.clip(np.floor(11 * (f2 + 1) * 0.5), 0, 10).astype(np.int64)
    return b0, b1 + 11, b2 + 22


def np_fpfh(pts, nrm, search, radius, max_nn):
    n = len(pts)
    ii, d2, valid = np_neighbours(pts, search, radius, max_nn)
    cnt = valid.sum(1)
    bs = np_pair_bins(pts[:, None, :], nrm[:, None, :], pts[ii], nrm[ii])
    use = valid.copy()
    use[:, 0] = False
    use &= (cnt > 1)[:, None]
    incr = 100.0 / np.maximum(cnt - 1, 1)
    rows = np.broadcast_to(np.arange(n)[:, None], ii.shape)
    spfh = np.zeros((n, 33))
    for b in bs:
        np.add.at(spfh, (rows[use], b[use]), np.broadcast_to(incr[:, None], ii.shape)[use])
    wgt = np.where(use & (d2 != 0), 1.0 / np.where(d2 == 0, 1, d2), 0.0)
    acc = np.einsum("nk,nkj->nj", wgt, spfh[ii])
    out = np.zeros((n, 33))
    for g in range(3):
        s = acc[:, 11 * g:11 * g + 11].sum(1)
        sc = np.where(s != 0, 100.0 / np.where(s == 0, 1, s), 0.0)
        out[:, 11 * g:11 * g + 11] = acc[:, 11 * g:11 * g + 11] * sc[:, None]
    out += spfh
    out[cnt <= 1] = 0
    return out


def np_normals(pts, idx, cnt):
    """centred covariance of the given neighbour sets, numpy eigh -> (normals, relative gap (l1 - l0) / l2)"""
    n = len(pts)
    out = np.zeros((n, 3))
    out[:, 2] = 1.0
    gap = np.full(n, np.inf)
    for i in range(n):
        m = int(cnt[i])
        if m < 3:
            continue
        q = pts[idx[i, :m]]
        c = q - q.mean(0)
        w, v = np.linalg.eigh(c.T @ c / m)
        out[i] = v[:, 0]
        gap[i] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
    return out, gap


# ---- clouds ---------------------------------------------------------------------------------------------------------
def three_surface_cloud(n=20000, seed=11, noise=0.002, normal_noise=0.02):
    """a noisy plane, a sphere and a cylinder, n points in all, unit normals with `normal_noise` of perturbation; seeded"""
    rng = np.random.default_rng(seed)
    a = n // 3
    b = n // 3
    c = n - a - b
    pl = np.stack([rng.uniform(-1, 1, a), rng.uniform(-1, 1, a), np.zeros(a)], 1)
    pl_n = np.tile([0.0, 0.0, 1.0], (a, 1))
    u = rng.normal(size=(b, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    sp = np.array([0.3, -0.2, 1.2]) + 0.6 * u
    th = rng.uniform(0, 2 * np.pi, c)
    cy_n = np.stack([np.cos(th), np.sin(th), np.zeros(c)], 1)
    cy = np.array([-1.0, 0.8, 0.0]) + 0.4 * cy_n + np.stack([np.zeros(c), np.zeros(c), rng.uniform(0.2, 1.6, c)], 1)
    pts = np.concatenate([pl, sp, cy]) + noise * rng.normal(size=(n, 3))
    nrm = np.concatenate([pl_n, u, cy_n]) + normal_noise * rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    perm = rng.permutation(n)
    return np.ascontiguousarray(pts[perm] + np.array([0.2, 0.1, 2.0])), np.ascontiguousarray(nrm[perm])


def lattice(side):
    g = np.stack(np.meshgrid(*[np.arange(side, dtype=np.float64)] * 3, indexing="ij"), -1)
    return g.reshape(-1, 3)


def group_sums_ok(rows, tol=1e-9):
    """every group of every row sums to 200, 100 or 0"""
    s = rows.reshape(len(rows), 3, 11).sum(2)
    return (np.minimum(np.minimum(np.abs(s - 200), np.abs(s - 100)), np.abs(s)) <= tol).all(1)


def differing_points(got, want, rtol=1e-9, atol=1e-9):
    """indices of the rows that differ beyond the tolerance"""
    return np.nonzero(~np.isclose(got, want, rtol=rtol, atol=atol).all(1))[0]
