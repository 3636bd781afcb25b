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


# The sizes at which the one-workgroup kernel changes its instantiation (1, 2, 4, 8 points per thread of 1024), each with its
# neighbours, and the first size of the tile path.
FPS_SINGLE_SEAMS = (1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192)
FPS_CROSSOVER = 8193
FPS_TILE = 512                       # points per tile of the tile path
FPS_SECOND_TRIP_N = 6144 * FPS_TILE + 77   # 6145 tiles: the step kernel's 1024 workgroups x 4 waves need a second trip


def fps_seam_cloud(n, seed=0):
    """the uniform cube with its two far corners at the END of the input: index n - 1 = (4, 4, 4), n - 2 = (-4, -4, -4).
    Both are among the first three samples, so the highest register slot, the last lane and the last tile decide the result"""
    p = np.random.default_rng(seed).uniform(-1, 1, (n, 3))
    p[n - 1] = 4.0
    p[n - 2] = -4.0
    return p


def fps_tie_steps(xyz, S):
    """the number of the first S - 1 steps at which more than one point holds the largest distance (the lowest index wins)"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    dist = np.full(len(xyz), np.inf)
    far, ties = 0, 0
    for _ in range(S - 1):
        dd = xyz - xyz[far]
        d = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
        dist = np.where(d < dist, d, dist)
        m = dist.max()
        ties += int((dist == m).sum() > 1)
        if m > 0:
            far = int(np.argmax(dist))
    return ties


def fps_unsorted_clouds(seed=0):
    """9001 points whose extent does not allow the tile path's sorting grid, so that every point, in input order, sits in
    the tiles: an extent that overflows to +inf, the same with a NaN and an inf row inside the tiles, a subnormal extent"""
    n = 9001
    a = np.random.default_rng(seed).uniform(-1, 1, (n, 3))
    a[100, 0] = 1.5e308
    a[7000, 0] = -1.5e308
    b = a.copy()
    b[5000, 1] = np.nan
    b[8999] = np.inf
    c = np.zeros((n, 3))
    c[:, 0] = np.arange(n) * 1e-300
    return {"inf_extent": a, "inf_extent_nonfinite": b, "subnormal_extent": c}


def fps_tile_edge_cloud(n_finite, nonfinite, seed=0):
    """n_finite uniform points and `nonfinite` rows with a NaN or an infinite coordinate among them, none at index 0 and the
    lowest one late: the finite points alone fill the tiles"""
    n = n_finite + nonfinite
    p = np.random.default_rng(seed).uniform(-1, 1, (n, 3))
    rows = [n - 700, n - 300, n - 1][:nonfinite]
    for k, r in enumerate(rows):
        p[r, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    return p


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
