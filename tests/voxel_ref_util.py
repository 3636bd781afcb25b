"""The plain-C restatement of the voxel down-sampling contract (tests/cpp/voxel_ref.c) built into a temporary directory and
loaded with ctypes, an independent numpy restatement of the same contract, and the clouds both voxel test files use."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

REF_ERRORS = {1: "[VoxelDownSample] voxel_size <= 0.", 2: "[VoxelDownSample] voxel_size is too small.",
              3: "non-finite point", 4: "voxel_size or bounds not finite"}


class RefError(Exception):
    def __init__(self, code, index=None):
        super().__init__(REF_ERRORS.get(code, str(code)))
        self.code = code
        self.index = index


def build_ref(tmpdir):
    so = os.path.join(str(tmpdir), "voxel_ref.so")
    if not os.path.exists(so):
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(HERE, "cpp", "voxel_ref.c"),
                        "-o", so, "-lm"], check=True)
    L = C.CDLL(so)
    L.voxel_ref.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double] + [C.c_void_p] * 7
    L.voxel_ref.restype = C.c_int

    def p(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    def voxel(xyz, voxel_size, normals=None, colors=None):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        normals = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3) if normals is not None else None
        colors = np.ascontiguousarray(colors, dtype=np.float64).reshape(-1, 3) if colors is not None else None
        n = len(xyz)
        cap = max(n, 1)
        o_xyz = np.empty((cap, 3))
        o_nrm = np.empty((cap, 3)) if normals is not None else None
        o_col = np.empty((cap, 3)) if colors is not None else None
        first = np.zeros(cap, dtype=np.uint64)
        p2v = np.zeros(cap, dtype=np.uint64)
        counts = np.zeros(cap, dtype=np.uint32)
        m = C.c_size_t(0)
        rc = L.voxel_ref(p(xyz), p(normals), p(colors), n, float(voxel_size), p(o_xyz), p(o_nrm), p(o_col), p(first), p(p2v),
                         p(counts), C.cast(C.byref(m), C.c_void_p))
        if rc != 0:
            raise RefError(rc, m.value if rc == 3 else None)
        k = m.value
        return {"points": o_xyz[:k].copy(), "normals": o_nrm[:k].copy() if normals is not None else None,
                "colors": o_col[:k].copy() if colors is not None else None, "first_index": first[:k].copy(),
                "point_to_voxel": p2v[:n].copy(), "counts": counts[:k].copy()}
    return voxel


def voxel_indices(xyz, voxel_size):
    """(indices (n, 3) int64, vmin): rules 2 and 3 with numpy's elementwise IEEE arithmetic; raises RefError(2)"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    v = np.float64(voxel_size)
    half = v * np.float64(0.5)
    vmin = xyz.min(axis=0) - half
    vmax = xyz.max(axis=0) + half
    if v * np.float64(2**31 - 1) < (vmax - vmin).max():
        raise RefError(2)
    return np.floor((xyz - vmin) / v).astype(np.int64), vmin


def voxel_numpy(xyz, voxel_size, normals=None, colors=None):
    """the contract once more: np.unique on the integer keys, then a Python loop that adds the members in index order"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    if not voxel_size > 0:
        raise RefError(1)
    n = len(xyz)
    if n == 0:
        return {"points": np.empty((0, 3)), "normals": None if normals is None else np.empty((0, 3)),
                "colors": None if colors is None else np.empty((0, 3)), "first_index": np.zeros(0, np.uint64),
                "point_to_voxel": np.zeros(0, np.uint64), "counts": np.zeros(0, np.uint32)}
    idx, _ = voxel_indices(xyz, voxel_size)
    _, inv = np.unique(idx, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    g = int(inv.max()) + 1
    first = np.full(g, n, dtype=np.int64)
    np.minimum.at(first, inv, np.arange(n))
    order = np.argsort(first, kind="stable")       # groups in ascending order of their lowest member
    row_of_group = np.empty(g, dtype=np.int64)
    row_of_group[order] = np.arange(g)
    p2v = row_of_group[inv]
    sums = np.zeros((g, 3))
    nsum = np.zeros((g, 3)) if normals is not None else None
    csum = np.zeros((g, 3)) if colors is not None else None
    counts = np.zeros(g, dtype=np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            j = p2v[i]
            sums[j] += xyz[i]
            if normals is not None and not np.isnan(normals[i]).any():
                nsum[j] += normals[i]
            if colors is not None:
                csum[j] += colors[i]
            counts[j] += 1
        div = counts.astype(np.float64)[:, None]
        return {"points": sums / div, "normals": None if normals is None else nsum / div,
                "colors": None if colors is None else csum / div, "first_index": first[order].astype(np.uint64),
                "point_to_voxel": p2v.astype(np.uint64), "counts": counts}


def bits(a):
    """an fp64 array as its raw bits (so that -0.0 and NaN compare by bits)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, exp, keys=("points", "normals", "colors")):
    """bit equality of two results' arrays (None == None)"""
    for k in keys:
        a, b = got.get(k), exp.get(k)
        if (a is None) != (b is None):
            return False
        if a is not None and (a.shape != b.shape or not np.array_equal(bits(a), bits(b))):
            return False
    return True


def extent(xyz):
    xyz = np.asarray(xyz).reshape(-1, 3)
    e = float((xyz.max(axis=0) - xyz.min(axis=0)).max())
    return e if e > 0 else 1.0


def faces_cloud(n, v, seed=3):
    """points on voxel faces by construction: a base point b (the minimum in every coordinate), vmin = b - v * 0.5, and
    every other point vmin + j * v with integer j in [1, 1000) per coordinate"""
    rng = np.random.default_rng(seed)
    b = rng.uniform(-1, 1, 3)
    vmin = b - np.float64(v) * 0.5
    j = rng.integers(1, 1000, (n - 1, 3)).astype(np.float64)
    return np.vstack([b[None, :], vmin + j * np.float64(v)])


def faces_fraction_moved(xyz, v):
    """the fraction of the points whose voxel differs between a division and a multiplication by the reciprocal"""
    v = np.float64(v)
    vmin = xyz.min(axis=0) - v * 0.5
    a = np.floor((xyz - vmin) / v)
    b = np.floor((xyz - vmin) * (np.float64(1.0) / v))
    return float((a != b).any(axis=1).mean())


# Member counts around the 64 members voxel_means_k stages at a time: one short of a batch, a full one, one into the second,
# two full ones, one into the third.
SEAM_HEAD = (1, 63, 64, 65, 128, 129)
# (m voxels, n points, head, sort passes): m on both sides of every change of (bit_width(m - 1) + 7) / 8.  The head is
# SEAM_HEAD wherever m voxels can hold it.
VOXEL_PASS_SEAMS = ((1, 65, (65,), 0), (2, 2049, (129,), 1), (256, 4097, SEAM_HEAD, 1), (257, 4096, SEAM_HEAD, 2),
                    (65_536, 70_000, SEAM_HEAD, 2), (65_537, 70_001, SEAM_HEAD, 3))
# element counts around the sort's round (64) and tile (2048, also the scan's tile) with m = min(n, 300) voxels, and around
# the bounds kernel's grid (1024 x 256 threads) and the 256 tile sums scan_sums_k takes at a time (256 x 2048 elements)
VOXEL_ELEMENT_SEAMS = (63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 262_144, 262_145, 524_287, 524_288, 524_289)


def seam_head(m, n):
    """SEAM_HEAD where m voxels of n points can hold it with one voxel left over for the highest cell, else no head"""
    return SEAM_HEAD if m > len(SEAM_HEAD) and n >= sum(SEAM_HEAD) + m - len(SEAM_HEAD) else ()


def voxel_seam_cloud(m, n, head=(), seed=0, highest_last=False):
    """(points, cell of every point): n points in exactly m voxels of size 1.0.  Voxel c is cell c of a lattice of side
    ceil(cbrt(m)) and holds exactly head[c] points for c < len(head); the other points are dealt at random over the other
    voxels, at least one each.  Points are cell + 0.5 + U[0, 0.4); index 0 is the lattice corner (0.5, 0.5, 0.5), so vmin
    is exactly 0; the order of the other points is shuffled.  highest_last: the highest cell holds one point, at index
    n - 1 and in the cell's far corner region (cell + 0.9), so the upper bounds come from the last element read"""
    rng = np.random.default_rng(seed)
    head = [int(h) for h in head]
    rest_cells = m - len(head)
    rest_points = n - sum(head)
    assert 1 <= m <= n and len(head) <= m and all(h >= 1 for h in head)
    assert rest_points >= rest_cells and (rest_cells > 0 or rest_points == 0)
    assert not highest_last or (m >= 2 and rest_cells >= (2 if rest_points > rest_cells else 1))
    counts = np.ones(m, dtype=np.int64)
    counts[:len(head)] = head
    free = rest_cells - (1 if highest_last else 0)            # cells that take the points left after one each
    extra = rest_points - rest_cells
    if extra:
        counts[len(head):len(head) + free] += np.bincount(rng.integers(0, free, extra), minlength=free)
    cell = np.repeat(np.arange(m), counts)
    assert len(cell) == n and cell[0] == 0
    side = 1
    while side ** 3 < m:
        side += 1
    ijk = np.stack([cell % side, (cell // side) % side, cell // (side * side)], 1).astype(np.float64)
    pts = ijk + 0.5 + rng.uniform(0, 0.4, (n, 3))
    pts[0] = 0.5
    last = n - 1 if highest_last else n                       # (the highest cell's single point is the last row already)
    if highest_last:
        pts[n - 1] = ijk[n - 1] + 0.9
    perm = np.concatenate([[0], 1 + rng.permutation(last - 1), np.arange(last, n)]).astype(np.int64)
    return np.ascontiguousarray(pts[perm]), cell[perm]


def seam_normals(cell, seed=0):
    """unit normals; in the voxels with exactly 65 and 129 members, the members at positions 0, 63 and 64 in ascending point
    index (the two sides of the first batch's end) get a NaN component, in the 129-member voxel 127 and 128 as well"""
    nrm = unit_normals(len(cell), seed)
    counts = np.bincount(cell)
    k = 0
    for size, positions in ((65, (0, 63, 64)), (129, (0, 63, 64, 127, 128))):
        for c in np.nonzero(counts == size)[0]:
            members = np.nonzero(cell == c)[0]
            for pos in positions:
                nrm[members[pos], k % 3] = np.nan
                k += 1
    return nrm


def unit_normals(n, seed=0, nan_rows=0):
    rng = np.random.default_rng(seed + 1000)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if nan_rows and n:
        rows = rng.integers(0, n, nan_rows)
        v[rows, rng.integers(0, 3, nan_rows)] = np.nan
        v[rows[: max(nan_rows // 4, 1)]] = np.nan
    return v
