"""The plain-C brute force of the ray casting contract (tests/cpp/raycast_ref.c) built into a temporary directory and loaded
with ctypes, an independent numpy float32 restatement of the same rules, and the scenes both ray casting test files use."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID = 0xFFFFFFFF
F32 = np.float32


class RefNonFinite(Exception):
    def __init__(self, index):
        super().__init__(f"transformed vertex {index} is not finite in fp32")
        self.index = index


def as_mesh(m):
    v, f = m
    return (np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(f, dtype=np.int32).reshape(-1, 3))


def as_poses(poses, n):
    p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    assert len(p) == n
    return p


def build_ref(tmpdir, openmp=False):
    """-> ray_cast(meshes, poses, (W, H, fx, fy, cx, cy)) -> dict(t_hit, geometry_ids, primitive_ids, normals, counts)"""
    so = os.path.join(str(tmpdir), "raycast_ref_omp.so" if openmp else "raycast_ref.so")
    if not os.path.exists(so):
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC"] + (["-fopenmp"] if openmp else []) +
                       [os.path.join(HERE, "cpp", "raycast_ref.c"), "-o", so, "-lm"], check=True)
    L = C.CDLL(so)
    L.raycast_ref.argtypes = [C.c_void_p] * 4 + [C.c_uint64, C.c_void_p, C.c_int, C.c_int] + [C.c_double] * 4 + [C.c_void_p] * 5
    L.raycast_ref.restype = C.c_int

    def ray_cast(meshes, poses, cam):
        meshes = [as_mesh(m) for m in meshes]
        poses = as_poses(poses, len(meshes))
        W, H, fx, fy, cx, cy = cam
        verts = np.ascontiguousarray(np.concatenate([m[0] for m in meshes] + [np.zeros((0, 3))]))
        tris = np.ascontiguousarray(np.concatenate([m[1] for m in meshes] + [np.zeros((0, 3), np.int32)]))
        voff = np.cumsum([0] + [len(m[0]) for m in meshes]).astype(np.uint64)
        toff = np.cumsum([0] + [len(m[1]) for m in meshes]).astype(np.uint64)
        t = np.empty((H, W), np.float32)
        g = np.empty((H, W), np.uint32)
        p = np.empty((H, W), np.uint32)
        nrm = np.empty((H, W, 3), np.float32)
        counts = np.zeros(3, np.uint64)
        rc = L.raycast_ref(verts.ctypes.data, voff.ctypes.data, tris.ctypes.data, toff.ctypes.data, len(meshes), poses.ctypes.data,
                           int(W), int(H), float(fx), float(fy), float(cx), float(cy), t.ctypes.data, g.ctypes.data, p.ctypes.data,
                           nrm.ctypes.data, counts.ctypes.data)
        if rc == 3:
            raise RefNonFinite(int(counts[0]))
        assert rc == 0
        return {"t_hit": t, "geometry_ids": g, "primitive_ids": p, "normals": nrm,
                "counts": {"mt_hits": int(counts[0]), "clause_rejected": int(counts[1]), "pixels_changed": int(counts[2])}}
    return ray_cast


def transform_f32(v, T):
    """rule 2: ((T0 x + T1 y) + T2 z) + T3 per row in fp64, rounded once"""
    out = np.empty((len(v), 3), np.float32)
    with np.errstate(all="ignore"):
        for r in range(3):
            s = T[r, 0] * v[:, 0] + T[r, 1] * v[:, 1]
            s = s + T[r, 2] * v[:, 2]
            s = s + T[r, 3]
            out[:, r] = s.astype(np.float32)
    return out


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def raycast_numpy(meshes, poses, cam, rows_per_chunk=8):
    """the rules once more, every operation a float32 array operation over (rays, triangles)"""
    meshes = [as_mesh(m) for m in meshes]
    poses = as_poses(poses, len(meshes))
    W, H, fx, fy, cx, cy = cam
    tv, geom, prim = [np.zeros((0, 3, 3), np.float32)], [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)]
    base = 0
    for g, (v, f) in enumerate(meshes):
        p = transform_f32(v, poses[g])
        bad = np.flatnonzero(~np.isfinite(p).all(axis=1))
        if len(bad):
            raise RefNonFinite(base + int(bad[0]))
        base += len(v)
        tv.append(p[f])
        geom.append(np.full(len(f), g, np.uint32))
        prim.append(np.arange(len(f), dtype=np.uint32))
    tv, geom, prim = np.concatenate(tv), np.concatenate(geom), np.concatenate(prim)
    nt = len(tv)
    v0, v1, v2 = ([tv[:, k, c][None, :] for c in range(3)] for k in range(3))
    e1 = [v1[c] - v0[c] for c in range(3)]
    e2 = [v2[c] - v0[c] for c in range(3)]
    s = [-v0[c] for c in range(3)]
    lo = [np.minimum(np.minimum(v0[c], v1[c]), v2[c]) for c in range(3)]
    hi = [np.maximum(np.maximum(v0[c], v1[c]), v2[c]) for c in range(3)]
    dxs = (((np.arange(W, dtype=np.float64) + 0.5) - cx) / fx).astype(np.float32)
    dys = (((np.arange(H, dtype=np.float64) + 0.5) - cy) / fy).astype(np.float32)
    t_hit = np.full(H * W, np.inf, np.float32)
    gid = np.full(H * W, INVALID, np.uint32)
    pid = np.full(H * W, INVALID, np.uint32)
    nrm = np.zeros((H * W, 3), np.float32)
    zero, one, inf, slack = F32(0), F32(1), F32(np.inf), F32(2.0 ** -16)
    with np.errstate(all="ignore"):
        q = _cross(s, e1)
        for y0 in range(0, H, rows_per_chunk):
            ys = np.arange(y0, min(H, y0 + rows_per_chunk))
            d = [np.tile(dxs, len(ys))[:, None], np.repeat(dys[ys], W)[:, None], np.ones((len(ys) * W, 1), np.float32)]
            if nt == 0:
                continue
            p = _cross(d, e2)
            det = _dot(e1, p)
            u = _dot(s, p) / det
            v = _dot(d, q) / det
            t = _dot(e2, q) / det
            ok = (det != zero) & (u >= zero) & (v >= zero) & (u + v <= one) & (t > zero) & (t < inf)
            a = np.zeros_like(t)
            b = np.full_like(t, inf)
            for c in range(3):
                nz = d[c] != zero
                inv = one / d[c]
                x, yv = lo[c] * inv, hi[c] * inv
                tn, tf = np.where(d[c] > zero, x, yv), np.where(d[c] > zero, yv, x)
                a = np.where(nz & (tn > a), tn, a)
                b = np.where(nz & (tf < b), tf, b)
                ok &= nz | ((lo[c] <= zero) & (zero <= hi[c]))
            ok &= (a <= b) & (t >= a - slack * b)
            tm = np.where(ok, t, inf)
            # the triangles are listed by (geometry id, primitive id): the first minimum is rule 4's winner
            k = np.argmin(tm, axis=1)
            rows = np.arange(len(k))
            hit = ok[rows, k]
            pix = (ys[0] * W + rows)[hit]
            kh = k[hit]
            t_hit[pix] = tm[rows, k][hit]
            gid[pix] = geom[kh]
            pid[pix] = prim[kh]
            a0, a1, a2 = tv[kh, 0], tv[kh, 1], tv[kh, 2]
            f1, f2 = a1 - a0, a2 - a0
            cr = np.stack(_cross(f1.T, f2.T), axis=1)
            l2 = _dot(cr.T, cr.T)
            good = (l2 > zero) & (l2 < inf)
            n = cr / np.sqrt(l2)[:, None]
            n[~good] = zero
            nrm[pix] = n
    return {"t_hit": t_hit.reshape(H, W), "geometry_ids": gid.reshape(H, W), "primitive_ids": pid.reshape(H, W),
            "normals": nrm.reshape(H, W, 3)}


KEYS = ("t_hit", "geometry_ids", "primitive_ids", "normals")


def bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, exp, keys=KEYS):
    """bit equality of the four maps (so that -0.0 and +0.0 differ)"""
    return all(got[k].shape == exp[k].shape and np.array_equal(bits32(got[k]), bits32(exp[k])) for k in keys)


def first_difference(got, exp):
    for k in KEYS:
        if got[k].shape != exp[k].shape:
            return f"{k}: shape {got[k].shape} != {exp[k].shape}"
        bad = np.argwhere(bits32(got[k]) != bits32(exp[k]))
        if len(bad):
            i = tuple(bad[0])
            return f"{k}: {len(bad)} entries differ, first at {i}: {got[k][i]!r} != {exp[k][i]!r}"
    return None


# ---- scenes ---------------------------------------------------------------------------------------------------------------
CAM = (64, 48, 60.0, 60.0, 31.5, 23.5)


def identity():
    return np.eye(4)


def pose(rx=0.0, ry=0.0, rz=0.0, t=(0.0, 0.0, 0.0)):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


def sphere(n_lat, n_lon, radius=0.5, center=(0.0, 0.0, 2.0)):
    """a latitude-longitude sphere: 2 n_lon (n_lat - 1) triangles"""
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            v.append((np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)))
    v.append((0.0, 0.0, -1.0))
    f = []
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    for j in range(n_lon):
        f.append((0, ring(1, j), ring(1, j + 1)))
        f.append((len(v) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            f.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    return np.array(v) * radius + np.array(center), np.array(f, dtype=np.int32)


def random_triangles(n, seed, size=0.4, depth=(1.0, 4.0)):
    """n triangles of a soup in front of the camera, three vertices each"""
    rng = np.random.default_rng(seed)
    c = np.column_stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-0.9, 0.9, n), rng.uniform(*depth, n)])
    v = (c[:, None, :] + rng.uniform(-size, size, (n, 3, 3))).reshape(-1, 3)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


TRI = (np.array([[-0.5, -0.4, 2.0], [0.6, -0.3, 2.2], [0.0, 0.5, 1.8]]), np.array([[0, 1, 2]], dtype=np.int32))
EMPTY = (np.zeros((0, 3)), np.zeros((0, 3), np.int32))
CAM_DX0 = (64, 48, 60.0, 60.0, 32.5, 23.5)      # pixel column 32 has dx == 0 exactly


def sphere_with_slivers():
    """a sphere with zero-area triangles (a vertex twice) and slivers along its edges mixed in, shuffled"""
    v, f = sphere(8, 12)
    rng = np.random.default_rng(5)
    extra = []
    for k in range(60):
        a, b = rng.integers(0, len(v), 2)
        extra.append((a, b, a if k % 3 == 0 else b))
    n0 = len(v)
    mid = (v[f[:40, 0]] + v[f[:40, 1]]) * 0.5 + rng.uniform(-1e-7, 1e-7, (40, 3))
    extra += [(f[k, 0], f[k, 1], n0 + k) for k in range(40)]
    f2 = np.vstack([f, np.array(extra, dtype=np.int32)])
    return np.vstack([v, mid]), f2[rng.permutation(len(f2))]


def scenes():
    """name -> (meshes, poses, camera, whether anything is hit): the scenes the GPU is judged on (tests/test_gpu_raycast.py),
    on which the C brute force and the numpy restatement must agree first (tests/test_raycast.py)"""
    I = identity()
    two = (np.vstack([TRI[0], TRI[0] + [0.3, 0.1, 0.4]]), np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32))
    ball = sphere(8, 12)
    crossing = (np.array([[-0.5, -0.5, -1.0], [0.5, -0.5, 1.0], [0.0, 0.5, 1.0]]), TRI[1])
    behind = (TRI[0] * [1, 1, -1], TRI[1])
    around = (np.array([[-1.0, -1.0, -0.5], [1.0, -1.0, 0.5], [0.0, 1.0, 0.1]]), TRI[1])
    through = (np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]]), TRI[1])       # the origin lies on it
    big = np.array([[-1e30, -1e30, 1e30], [1e30, -1e30, 1e30], [0.0, 1e30, 1e30]])
    small = np.array([[-1e-30, -1e-30, 1e-30], [1e-30, -1e-30, 1e-30], [0.0, 1e-30, 1e-30]])
    T = pose(0.2, 0.1, 0.0, (0.05, -0.02, 0.1))
    rng = np.random.default_rng(40)
    forty_poses = [pose(*rng.uniform(-1, 1, 3), t=(rng.uniform(-0.9, 0.9), rng.uniform(-0.7, 0.7), rng.uniform(1.5, 3.0))) for _ in range(40)]
    off_tile = [sphere(8, 12, 0.8), random_triangles(60, 2)]
    s = {
        "1 triangle": ([TRI], [I], CAM, True),
        "1 triangle, posed": ([TRI], [pose(0.4, -0.3, 1.0, (0.2, 0.1, 0.5))], CAM, True),
        "2 triangles": ([two], [I], CAM, True),
        "2 meshes of 1 triangle": ([TRI, TRI], [I, pose(0, 0, 0.5, (0.1, 0.0, -0.3))], CAM, True),
        "300 identical triangles": ([(np.tile(TRI[0], (300, 1)), np.arange(900, dtype=np.int32).reshape(300, 3))], [I], CAM, True),
        "identical meshes, same pose": ([ball, ball], [T, T], CAM, True),
        "empty mesh between": ([sphere(6, 8, 0.3, (-0.4, 0, 2)), EMPTY, sphere(6, 8, 0.3, (0.4, 0, 2))], [I] * 3, CAM, True),
        "only empty meshes": ([EMPTY, EMPTY], [I] * 2, CAM, False),
        "crossing z = 0": ([crossing], [I], CAM, True),
        "behind the camera": ([behind], [I], CAM, False),
        "behind, crossing, in front": ([behind, crossing, TRI], [I] * 3, CAM, True),
        "around the origin": ([around], [I], CAM, True),
        "through the origin": ([through], [I], CAM, False),
        "origin triangles and a sphere": ([around, through, sphere(5, 7)], [I] * 3, CAM, True),
        "slivers and zero area": ([sphere_with_slivers()], [pose(0.3, 0.2, 0.1)], CAM, True),
        "1e30, 1e-30 and 1": ([(np.vstack([big, small, TRI[0]]), np.arange(9, dtype=np.int32).reshape(3, 3))], [I], CAM, True),
        "1e30": ([(big, TRI[1])], [I], CAM, False),
        "1e-30": ([(small, TRI[1])], [I], CAM, False),
        "dx = 0": ([ball, random_triangles(100, 8)], [I] * 2, CAM_DX0, True),
        "dx = 0 and dy = 0": ([sphere(8, 12, 0.5, (0, 0, 2))], [I], (64, 48, 60.0, 60.0, 32.5, 24.5), True),
        "1 x 1": (off_tile, [I] * 2, (1, 1, 1.0, 1.0, 0.4, 0.6), True),
        "7 x 5": (off_tile, [I] * 2, (7, 5, 6.0, 6.0, 3.1, 2.2), True),
        "65 x 9": (off_tile, [I] * 2, (65, 9, 60.0, 10.0, 32.0, 4.0), True),
        "40 small meshes": ([sphere(4, 6, 0.12, (0, 0, 0)) for _ in range(40)], forty_poses, CAM, True),
    }
    for n in (255, 256, 257):
        s[f"{n} triangles"] = ([random_triangles(n, n)], [I], CAM, True)
    return s


BATCH_MESHES = lambda: [sphere(8, 12), random_triangles(150, 9)]   # noqa: E731
BATCH_FRAMES = lambda: [[pose(0.1 * k, 0.2, 0.0, (0.1 * k, 0.0, 0.2 * k)), pose(0.0, 0.0, 0.3 * k)] for k in range(3)]   # noqa: E731


def golden_obj(divide=1):
    """the reference's ray_cast_rendering example: (mesh, the two poses, the camera with the intrinsics divided by `divide`)"""
    d = np.load(os.path.join(HERE, "golden", "raycast_obj.npz"))
    mesh = (d["vertices"].astype(np.float64) * float(d["scale"]), d["triangles"].astype(np.int32))
    w, h, fx, fy, cx, cy = d["intrinsic"]
    return mesh, d["poses"].astype(np.float64), (int(w) // divide, int(h) // divide, fx / divide, fy / divide, cx / divide, cy / divide)
