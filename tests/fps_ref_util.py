"""The plain-C restatement of FarthestPointSampling (tests/cpp/fps_ref.c) built into a temporary directory and loaded with
ctypes, a numpy restatement of the same contract, and the quirk clouds both test files use."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def build_ref(tmpdir, order=0):
    so = os.path.join(str(tmpdir), f"fps_ref_{order}.so")
    if not os.path.exists(so):
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", f"-DORDER={order}",
                        os.path.join(HERE, "cpp", "fps_ref.c"), "-o", so], check=True)
    L = C.CDLL(so)
    L.fps_ref.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
    L.fps_ref.restype = None

    def fps(xyz, S):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        out = np.zeros(S, dtype=np.uint64)
        dist = np.empty(max(len(xyz), 1))
        L.fps_ref(xyz.ctypes.data, len(xyz), S, out.ctypes.data, dist.ctypes.data)
        return out
    return fps


def fps_numpy(xyz, S):
    """the contract once more, vectorised over j (numpy rounds every product and sum on its own: order 0)"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    dist = np.full(len(xyz), np.inf)
    out = np.zeros(S, dtype=np.uint64)
    far = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(S):
            out[i] = far
            dd = xyz - xyz[far]
            d = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
            dist = np.where(d < dist, d, dist)
            m = dist.max()
            if m > 0:
                far = int(np.argmax(dist))   # (the first index of the maximum)
    return out


def shaped_clouds(n, seed=0):
    """uniform cube, thin plane patch, sphere shell, clusters with exact duplicates, integer lattice, collinear"""
    rng = np.random.default_rng(seed)
    out = {"cube": rng.uniform(-1, 1, (n, 3))}
    p = rng.uniform(-1, 1, (n, 3))
    p[:, 2] = 1e-4 * rng.standard_normal(n)
    out["plane"] = p
    v = rng.standard_normal((n, 3))
    out["sphere"] = v / np.linalg.norm(v, axis=1, keepdims=True) * 2.5
    centres = rng.uniform(-5, 5, (max(n // 50, 1), 3))
    c = centres[rng.integers(0, len(centres), n)] + 0.05 * rng.standard_normal((n, 3))
    dup = rng.integers(0, n, n // 4)
    c[rng.integers(0, n, n // 4)] = c[dup]
    out["clusters"] = c
    side = max(int(round(n ** (1 / 3))) + 1, 2)
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 3)
    out["lattice"] = g[rng.permutation(len(g))[:n]].astype(np.float64)
    t = rng.uniform(-3, 3, n)
    out["collinear"] = np.stack([t, 2 * t + 1, -t], 1)
    return out


def quirk_clouds(seed=0):
    """all points equal; k distinct positions (S > k repeats the last index); NaN at index 0; NaN / inf rows at j > 0;
    |coord| ~ 1e155 (the squares overflow); signed zeros"""
    rng = np.random.default_rng(seed)
    out = {"all_equal": np.tile([[0.5, -1.25, 3.0]], (300, 1))}
    pos = rng.uniform(-1, 1, (5, 3))
    out["k_distinct"] = pos[rng.integers(0, 5, 400)]
    a = rng.uniform(-1, 1, (300, 3))
    a[0, 1] = np.nan
    out["nan_first"] = a
    b = rng.uniform(-1, 1, (700, 3))
    b[17, 0] = np.nan
    b[40, 2] = np.inf
    b[333, 1] = -np.inf
    b[600] = np.nan
    out["nonfinite_later"] = b
    c = rng.uniform(-1, 1, (600, 3)) * 1e155
    c[::7] *= 1e-150
    out["overflow"] = c
    z = rng.choice([0.0, -0.0, 1.0, -1.0], (500, 3))
    out["signed_zero"] = z
    return out
