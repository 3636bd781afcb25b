"""The plain-C restatement of the ICP contract (tests/cpp/icp_ref.c) built into a temporary directory and loaded with ctypes, the
multi-scale restatement on top of it (its levels come from tests/cpp/voxel_ref.c), an independent numpy restatement, and the
clouds and cases both ICP test files use."""
import ctypes as C
import os
import subprocess

import numpy as np

import voxel_ref_util as vu

HERE = os.path.dirname(os.path.abspath(__file__))

NO_NORMALS = ("TransformationEstimationPointToPlane and TransformationEstimationColoredICP require pre-computed normal vectors "
              "for target PointCloud.")
INVALID_DISTANCE = "Invalid max_correspondence_distance."


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class IcpRef:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "icp_ref.so")
        if not os.path.exists(so):
            subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(HERE, "cpp", "icp_ref.c"), "-o", so,
                            "-lm"], check=True)
        L = C.CDLL(so)
        L.icp_ref.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_int,
                              C.c_double, C.c_double, C.c_int] + [C.c_void_p] * 7
        L.icp_ref.restype = C.c_int
        L.icp_ref_correspondences.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_void_p]
        L.icp_ref_correspondences.restype = C.c_int
        self.L = L
        self.voxel = vu.build_ref(tmpdir)

    def icp(self, src, dst, max_dist, init=None, max_iteration=30, dst_normals=None, order=1, rel_fitness=1e-6, rel_rmse=1e-6):
        """-> dict(T, fitness, inlier_rmse, correspondences, iterations, converged, corr); dst_normals=None: point-to-point"""
        src, dst = _f(src).reshape(-1, 3), _f(dst).reshape(-1, 3)
        nrm = _f(dst_normals).reshape(-1, 3) if dst_normals is not None else None
        Ti = _f(init if init is not None else np.eye(4)).reshape(16).copy()
        T = np.zeros(16)
        fit, rm = C.c_double(0), C.c_double(0)
        cnt = C.c_uint64(0)
        it, conv = C.c_int(0), C.c_int(0)
        corr = np.full(max(len(src), 1), -1, dtype=np.int64)
        rc = self.L.icp_ref(_p(src), len(src), _p(dst), _p(nrm), len(dst), float(max_dist), _p(Ti), int(max_iteration),
                            rel_fitness, rel_rmse, int(order), _p(T), C.cast(C.byref(fit), C.c_void_p),
                            C.cast(C.byref(rm), C.c_void_p), C.cast(C.byref(cnt), C.c_void_p), C.cast(C.byref(it), C.c_void_p),
                            C.cast(C.byref(conv), C.c_void_p), _p(corr))
        if rc != 0:
            raise RuntimeError(INVALID_DISTANCE if rc == 1 else "icp_ref: out of memory")
        return {"T": T.reshape(4, 4), "fitness": fit.value, "inlier_rmse": rm.value, "correspondences": cnt.value,
                "iterations": it.value, "converged": conv.value, "corr": corr[: len(src)]}

    def correspondences(self, src, dst, max_dist, T):
        src, dst = _f(src).reshape(-1, 3), _f(dst).reshape(-1, 3)
        corr = np.full(max(len(src), 1), -1, dtype=np.int64)
        rc = self.L.icp_ref_correspondences(_p(src), len(src), _p(dst), len(dst), float(max_dist), _p(_f(T).reshape(16).copy()),
                                            _p(corr))
        assert rc == 0
        return corr[: len(src)]

    def information(self, src, dst, max_dist, T):
        """GetInformationMatrixFromPointClouds: sum of G^T G over the matched target points, G = [-[t]x | I]"""
        corr = self.correspondences(src, dst, max_dist, T)
        t = _f(dst).reshape(-1, 3)[corr[corr >= 0]]
        G = np.zeros((len(t), 3, 6))
        x, y, z = t[:, 0], t[:, 1], t[:, 2]
        G[:, 0, 1], G[:, 0, 2] = z, -y
        G[:, 1, 0], G[:, 1, 2] = -z, x
        G[:, 2, 0], G[:, 2, 1] = y, -x
        G[:, 0, 3] = G[:, 1, 4] = G[:, 2, 5] = 1.0
        return np.einsum("nki,nkj->ij", G, G), int((corr >= 0).sum())

    def multi_scale(self, src, dst, voxel_sizes, max_iters, max_dist, init=None, dst_normals=None, order=1):
        """ReconstructionPipeline::MultiScaleICP restated: per level both clouds through voxel_ref.c, icp_ref seeded with the
        previous pose, then the information matrix of the original clouds at 1.4 voxel_sizes[-1]"""
        T = np.eye(4) if init is None else _f(init).reshape(4, 4)
        levels = []
        for v, it in zip(voxel_sizes, max_iters):
            s = self.voxel(src, v)
            d = self.voxel(dst, v, normals=dst_normals)
            r = self.icp(s["points"], d["points"], max_dist, T, it, d["normals"] if dst_normals is not None else None, order)
            r["n_src"], r["n_dst"] = len(s["points"]), len(d["points"])
            levels.append(r)
            T = r["T"]
        info, n_info = self.information(src, dst, float(voxel_sizes[-1]) * 1.4, T)
        return {"T": T, "info": info, "n_info": n_info, "levels": levels}


# ---- the numpy restatement (brute-force search, numpy's solvers): the independent cross-check of icp_ref.c
def _nearest_numpy(mov, dst, r2):
    """exhaustive over the finite target points whose x lies within the radius (plus a margin) of the moving point's: no other
    can be a correspondence -- d2 >= dx * dx holds in floating point too, rounding being monotone -- and a 16 000-point pair
    takes a second instead of a quarter of a minute"""
    corr = np.full(len(mov), -1, dtype=np.int64)
    d2s = np.zeros(len(mov))
    ok = np.nonzero(np.isfinite(dst).all(axis=1))[0]
    ok = ok[np.argsort(dst[ok, 0], kind="stable")]
    xs, reach = dst[ok, 0], 1.001 * np.sqrt(r2)
    for i, p in enumerate(mov):
        if not np.isfinite(p).all():
            continue
        cand = np.sort(ok[np.searchsorted(xs, p[0] - reach):np.searchsorted(xs, p[0] + reach, side="right")])
        if len(cand) == 0:
            continue
        d = p - dst[cand]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        k = int(np.argmin(d2))            # (the first index of the minimum, cand ascending: lowest index on ties)
        if d2[k] < r2:
            corr[i], d2s[i] = cand[k], d2[k]
    return corr, d2s


def icp_numpy(src, dst, max_dist, init=None, max_iteration=30, dst_normals=None):
    src, dst = _f(src).reshape(-1, 3), _f(dst).reshape(-1, 3)
    T = np.eye(4) if init is None else _f(init).reshape(4, 4).copy()
    mov = src @ T[:3, :3].T + T[:3, 3] if not np.array_equal(T, np.eye(4)) else src.copy()
    r2 = float(max_dist) * float(max_dist)

    def result():
        corr, d2 = _nearest_numpy(mov, dst, r2)
        c = int((corr >= 0).sum())
        return corr, c, c / len(src), (np.sqrt(d2[corr >= 0].sum() / c) if c else 0.0)

    corr, cnt, fit, rm = result()
    it, conv = 0, 0
    while it < max_iteration:
        U = np.eye(4)
        m = corr >= 0
        if cnt:
            s, t = mov[m], dst[corr[m]]
            if dst_normals is not None:
                n = _f(dst_normals).reshape(-1, 3)[corr[m]]
                r = ((s - t) * n).sum(axis=1)
                J = np.hstack([np.cross(s, n), n])
                A, b = J.T @ J, J.T @ r
                det = np.linalg.det(A)
                if np.isfinite(det) and abs(det) >= 1e-6:
                    x = np.linalg.solve(A, -b)
                    c, sn = np.cos(x[:3]), np.sin(x[:3])
                    Rx = np.array([[1, 0, 0], [0, c[0], -sn[0]], [0, sn[0], c[0]]])
                    Ry = np.array([[c[1], 0, sn[1]], [0, 1, 0], [-sn[1], 0, c[1]]])
                    Rz = np.array([[c[2], -sn[2], 0], [sn[2], c[2], 0], [0, 0, 1]])
                    U[:3, :3], U[:3, 3] = Rz @ Ry @ Rx, x[3:]
            else:
                ms, mt = s.mean(axis=0), t.mean(axis=0)
                Uu, _, Vt = np.linalg.svd((t - mt).T @ (s - ms) / len(s))
                S = np.diag([1.0, 1.0, np.sign(np.linalg.det(Uu) * np.linalg.det(Vt))])
                U[:3, :3] = Uu @ S @ Vt
                U[:3, 3] = mt - U[:3, :3] @ ms
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
def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def truth_pose(angle_deg=40.0, axis=(1, 1, 1), t=(0.3, -0.1, 0.2)):
    a = _unit(axis)
    th = np.deg2rad(angle_deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


def offset_pose(T, angle_deg, shift):
    """the truth plus a small offset: a rotation about (1, -2, 0.5) and a translation"""
    D = truth_pose(angle_deg, (1.0, -2.0, 0.5), shift)
    return D @ T


def icp_pair(n, seed=5, sigma=0.001):
    """The six patches of synth.registration_pair_c4 -- three planar (half-size 0.3), three spherical (radius 0.25), centres in
    [-0.7, 0.7]^3 -- with analytic unit normals; the target is the rigidly moved source plus `sigma` noise, permuted, its
    normals rotated.  -> dict(src, src_normals, dst, dst_normals, T, perm)"""
    rng = np.random.default_rng(seed)
    per = n // 6
    pts, nrm = [], []
    for k in range(6):
        m = per if k < 5 else n - 5 * per
        centre = rng.uniform(-0.7, 0.7, size=3)
        if k % 2 == 0:
            normal = _unit(rng.normal(size=3))
            a = _unit(np.cross(normal, [1.0, 0.0, 0.0] if abs(normal[0]) < 0.9 else [0.0, 1.0, 0.0]))
            b = np.cross(normal, a)
            uv = rng.uniform(-0.3, 0.3, size=(m, 2))
            pts.append(centre + uv[:, :1] * a + uv[:, 1:] * b)
            nrm.append(np.tile(normal, (m, 1)))
        else:
            u = rng.normal(size=(m, 3))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            pts.append(centre + 0.25 * u)
            nrm.append(u)
    order = rng.permutation(n)
    src, sn = np.concatenate(pts)[order], np.concatenate(nrm)[order]
    T = truth_pose()
    perm = rng.permutation(n)
    dst = (src @ T[:3, :3].T + T[:3, 3] + rng.normal(0, sigma, size=(n, 3)))[perm]
    dn = (sn @ T[:3, :3].T)[perm]
    c = np.ascontiguousarray
    return {"src": c(src), "src_normals": c(sn), "dst": c(dst), "dst_normals": c(dn), "T": T, "perm": perm}


def case(name):
    """The inputs of the GPU tests' cases -> dict(src, dst, dst_normals, max_dist, init, max_iteration[, T])"""
    if name in ("refine", "no_convergence"):
        p = icp_pair(6001, seed=11)
        return dict(src=p["src"], dst=p["dst"], dst_normals=p["dst_normals"], max_dist=0.02, T=p["T"],
                    init=offset_pose(p["T"], 1.0, (0.008, -0.006, 0.005)), max_iteration=30 if name == "refine" else 2)
    if name == "small":
        p = icp_pair(601, seed=12)
        return dict(src=p["src"], dst=p["dst"], dst_normals=p["dst_normals"], max_dist=0.06, T=p["T"],
                    init=offset_pose(p["T"], 1.0, (0.01, -0.005, 0.008)), max_iteration=30)
    if name == "identity_init":
        # no initial pose (the iteration without a pending update): the source already moved close to the target
        p = icp_pair(601, seed=12)
        src = p["src"] @ p["T"][:3, :3].T + p["T"][:3, 3] + 0.004
        return dict(src=np.ascontiguousarray(src), dst=p["dst"], dst_normals=p["dst_normals"], max_dist=0.06, T=np.eye(4),
                    init=None, max_iteration=30)
    if name == "duplicates":
        # the first 300 target rows once more at the end, their normals turned by 20 degrees: every query that matches one
        # of them meets an exact tie, and only the lower index carries the right normal
        p = icp_pair(1201, seed=13)
        R = truth_pose(20.0, (0.3, 1.0, -0.2), (0, 0, 0))[:3, :3]
        dst = np.vstack([p["dst"], p["dst"][:300]])
        dn = np.vstack([p["dst_normals"], p["dst_normals"][:300] @ R.T])
        return dict(src=p["src"], dst=np.ascontiguousarray(dst), dst_normals=np.ascontiguousarray(dn), max_dist=0.05, T=p["T"],
                    init=offset_pose(p["T"], 0.8, (0.008, -0.004, 0.006)), max_iteration=30)
    if name == "nonfinite":
        p = icp_pair(1501, seed=14)
        src, dst, dn = p["src"].copy(), p["dst"].copy(), p["dst_normals"].copy()
        src[[3, 700, 1500]] = np.nan
        src[41, 1] = np.nan
        dst[[5, 900]] = np.inf
        dst[77, 2] = -np.inf
        init = offset_pose(p["T"], 0.5, (0.004, -0.002, 0.003))
        # a NaN normal on a target point that IS matched under the initial pose: the twin of source point 10
        j = int(np.nonzero(p["perm"] == 10)[0][0])
        dn[j, 0] = np.nan
        return dict(src=src, dst=dst, dst_normals=dn, max_dist=0.05, T=p["T"], init=init, max_iteration=30, nan_normal_at=j)
    if name == "no_correspondences":
        p = icp_pair(901, seed=15)
        return dict(src=p["src"], dst=p["dst"] + 100.0, dst_normals=p["dst_normals"], max_dist=0.05, T=p["T"],
                    init=offset_pose(p["T"], 0.5, (0.004, -0.002, 0.003)), max_iteration=30)
    raise KeyError(name)


CASES = ("refine", "small", "no_convergence", "duplicates", "nonfinite", "no_correspondences", "identity_init")


def sized_case(n_src, max_iteration=3):
    """the iteration kernels' seams: n_src moving points (the first rows of a pair of n_src + 40), at most 3 iterations"""
    p = icp_pair(n_src + 40, seed=40 + n_src % 7)
    return dict(src=np.ascontiguousarray(p["src"][:n_src]), dst=p["dst"], dst_normals=p["dst_normals"], T=p["T"],
                max_dist=0.08 if n_src < 1000 else 0.02, init=offset_pose(p["T"], 0.5, (0.004, -0.002, 0.003)),
                max_iteration=max_iteration)

MULTI_VOXEL = 0.05


def multi_case(n=20000):
    """The multi-scale tests' input: voxel 0.05, max_correspondence_distance 1.4 voxel"""
    p = icp_pair(n, seed=21)
    v = float(np.float32(MULTI_VOXEL))
    return dict(src=p["src"], dst=p["dst"], dst_normals=p["dst_normals"], T=p["T"], voxel=v, max_dist=v * 1.4,
                init=offset_pose(p["T"], 1.5, (0.02, -0.01, 0.015)))


def levels_of(v, three):
    v = np.float32(v)
    return ([float(v), float(v / np.float32(2)), float(v / np.float32(4))], [50, 30, 15]) if three else ([float(v)], [50])
