"""The plain-C restatement of ProximityExtractor::Segment (tests/cpp/proximity_ref.c) built into a temporary directory and
loaded with ctypes, the scipy partition it is checked against, and the clouds the proximity tests share."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = {"distance": 1, "normals": 2, "distance_normals": 3}


def build_ref(tmpdir):
    so = os.path.join(str(tmpdir), "proximity_ref.so")
    if not os.path.exists(so):
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(HERE, "cpp", "proximity_ref.c"),
                        "-o", so, "-lm"], check=True)
    L = C.CDLL(so)
    P = C.c_void_p
    L.prox_ref_segment.argtypes = [P, P, C.c_size_t, C.c_double, C.c_int, C.c_double, C.c_double, C.c_size_t, C.c_size_t,
                                   P, P, P, P]
    L.prox_ref_segment_nn.argtypes = [P, P, C.c_size_t, P, P, C.c_int, C.c_double, C.c_double, C.c_size_t, C.c_size_t,
                                      P, P, P, P]
    L.prox_ref_dist_test.argtypes = [P, C.c_size_t, C.c_double, C.c_int, P]
    L.prox_ref_angle_test.argtypes = [P, C.c_size_t, C.c_double, P]
    for f in (L.prox_ref_segment, L.prox_ref_segment_nn, L.prox_ref_dist_test, L.prox_ref_angle_test):
        f.restype = None
    return Ref(L)


class Ref:
    def __init__(self, L):
        self.L = L

    @staticmethod
    def _out(n):
        return (np.zeros(n + 1, np.uint64), np.zeros(max(n, 1), np.uint64), C.c_size_t(0), np.zeros(max(n, 1), np.uint64))

    @staticmethod
    def _result(n, off, idx, k, lab):
        k = k.value
        return [idx[off[c]:off[c + 1]].astype(np.int64).tolist() for c in range(k)], lab[:n].astype(np.int64)

    def segment(self, xyz, radius, kind, dist=0.0, angle=0.0, normals=None, min_size=1, max_size=2**64 - 1):
        """-> (clusters as list[list[int]], labels)"""
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
        n = len(xyz)
        off, idx, k, lab = self._out(n)
        self.L.prox_ref_segment(xyz.ctypes.data, None if nrm is None else nrm.ctypes.data, n, radius, KINDS[kind], dist,
                                angle, min_size, max_size, off.ctypes.data, idx.ctypes.data, C.addressof(k), lab.ctypes.data)
        return self._result(n, off, idx, k, lab)

    def segment_nn(self, xyz, lists, kind, dist=0.0, angle=0.0, normals=None, min_size=1, max_size=2**64 - 1):
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
        n = len(xyz)
        nn_off = np.zeros(n + 1, np.uint64)
        nn_off[1:] = np.cumsum([len(l) for l in lists])
        nn_idx = np.array([j for l in lists for j in l] or [0], np.uint64)
        off, idx, k, lab = self._out(n)
        self.L.prox_ref_segment_nn(xyz.ctypes.data, None if nrm is None else nrm.ctypes.data, n, nn_off.ctypes.data,
                                   nn_idx.ctypes.data, KINDS[kind], dist, angle, min_size, max_size, off.ctypes.data,
                                   idx.ctypes.data, C.addressof(k), lab.ctypes.data)
        return self._result(n, off, idx, k, lab)

    def dist_test(self, d2, t, distance_normals):
        d2 = np.ascontiguousarray(d2, np.float64)
        out = np.zeros(len(d2), np.uint8)
        self.L.prox_ref_dist_test(d2.ctypes.data, len(d2), t, int(distance_normals), out.ctypes.data)
        return out.astype(bool)

    def angle_test(self, dot, angle_deg):
        dot = np.ascontiguousarray(dot, np.float64)
        out = np.zeros(len(dot), np.uint8)
        self.L.prox_ref_angle_test(dot.ctypes.data, len(dot), angle_deg, out.ctypes.data)
        return out.astype(bool)


def scipy_partition(xyz, radius, dist=None):
    """connected components of the radius graph (Distance evaluator when dist is given): the canonical order"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    xyz = np.asarray(xyz, np.float64)
    n = len(xyz)
    fin = np.isfinite(xyz).all(1)
    idx = np.flatnonzero(fin)
    pairs = cKDTree(xyz[fin]).query_pairs(radius * 1.0001, output_type="ndarray")
    a, b = idx[pairs[:, 0]], idx[pairs[:, 1]]
    d = xyz[a] - xyz[b]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    keep = d2 <= radius * radius
    if dist is not None:
        keep &= np.sqrt(d2) < dist
    g = coo_matrix((np.ones(keep.sum()), (a[keep], b[keep])), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    return canonical(lab)


def canonical(lab, min_size=1):
    """component labels -> clusters in the canonical order (size desc, smallest index asc), indices ascending"""
    lab = np.asarray(lab)
    order = np.argsort(lab, kind="stable")
    cuts = np.flatnonzero(np.diff(lab[order])) + 1
    groups = [g for g in np.split(order, cuts) if len(g) >= min_size]
    groups.sort(key=lambda g: (-len(g), g[0]))
    return [g.tolist() for g in groups]


def golden_ply():
    from misc3d_amd import io
    return np.asarray(io.read_ply(os.path.join(HERE, "golden", "segmentation_test.ply"))["points"], np.float64)


def voxel_average(xyz, voxel):
    """Open3D-style voxel_down_sample (mean of each voxel's points), voxels in the order of their keys"""
    key = np.floor((xyz - xyz.min(0)) / voxel).astype(np.int64)
    _, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv)
    return np.stack([np.bincount(inv, xyz[:, k]) / cnt for k in range(3)], 1)


def pca_normals(xyz, radius, k=15, view=(0.0, 0.0, 0.0)):
    """unit normals from the covariance of up to k nearest points within radius, oriented towards `view`"""
    from scipy.spatial import cKDTree
    t = cKDTree(xyz)
    dd, ii = t.query(xyz, k=min(k, len(xyz)), distance_upper_bound=radius)
    out = np.zeros_like(xyz)
    for i in range(len(xyz)):
        nb = ii[i][np.isfinite(dd[i])]
        q = xyz[nb] - xyz[nb].mean(0)
        w, v = np.linalg.eigh(q.T @ q if len(nb) >= 3 else np.eye(3))
        nrm = v[:, 0]
        if np.dot(nrm, np.asarray(view) - xyz[i]) < 0:
            nrm = -nrm
        out[i] = nrm
    return out
