"""The plain-C restatement of the contract "PPF model preprocessing" (tests/cpp/ppf_train_ref.c: the reference's heap walk under
the O2 order, its FIFO sampler, B1 / B2 / B4, SampleWithoutDuplicate) built into a temporary directory and loaded with ctypes; an
independent judge of the orientation in python (Kruskal under O2, then a breadth-first pass); and the input families the CPU and
the GPU tests share."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class TrainRef:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "ppf_train_ref.so")
        if not os.path.exists(so):
            subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(HERE, "cpp", "ppf_train_ref.c"), "-o", so,
                            "-lm"], check=True)
        L = C.CDLL(so)
        L.ptr_orient.restype = None
        L.ptr_orient.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ptr_orient_timed.restype = None
        L.ptr_orient_timed.argtypes = L.ptr_orient.argtypes + [C.c_void_p, C.c_void_p]
        L.ptr_sample.restype = C.c_size_t
        L.ptr_sample.argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_size_t, C.c_void_p]
        L.ptr_box.restype = None
        L.ptr_box.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.ptr_derive.restype = None
        L.ptr_derive.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p]
        L.ptr_prepare_normals.restype = C.c_size_t
        L.ptr_prepare_normals.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
        L.ptr_reference_indices.restype = None
        L.ptr_reference_indices.argtypes = [C.c_size_t, C.c_size_t, C.c_uint32, C.c_void_p]
        self.L = L

    def orient(self, points, normals, radius, seed):
        """-> (normals, parent, dict(rounds, tree_edges, component, flips))"""
        xyz, nrm = _f(points), _f(normals)
        out, parent, st = np.zeros_like(xyz), np.zeros(len(xyz), np.int64), np.zeros(4, np.uint64)
        self.L.ptr_orient(_p(xyz), _p(nrm), len(xyz), float(radius), int(seed), _p(out), _p(parent), _p(st))
        return out, parent, dict(zip(STATS, (int(v) for v in st)))

    def orient_timed(self, points, normals, radius, seed):
        """orient + dict(ms_lists, ms_walk, ms_rounds_count, list_entries): the walk's time apart from its brute-force lists"""
        xyz, nrm = _f(points), _f(normals)
        out, parent, st = np.zeros_like(xyz), np.zeros(len(xyz), np.int64), np.zeros(4, np.uint64)
        ms, e = np.zeros(3), np.zeros(1, np.uint64)
        self.L.ptr_orient_timed(_p(xyz), _p(nrm), len(xyz), float(radius), int(seed), _p(out), _p(parent), _p(st), _p(ms), _p(e))
        return out, parent, dict(zip(STATS, (int(v) for v in st))), dict(ms_lists=ms[0], ms_walk=ms[1], ms_rounds_count=ms[2], list_entries=int(e[0]))

    def sample(self, points, step, seed):
        xyz = _f(points)
        out = np.zeros(len(xyz), np.uint64)
        k = self.L.ptr_sample(_p(xyz), len(xyz), float(step), int(seed), _p(out))
        return out[:k].astype(np.int64)

    def box(self, points):
        xyz, c, e = _f(points), np.zeros(3), np.zeros(3)
        self.L.ptr_box(_p(xyz), len(xyz), _p(c), _p(e))
        return c, e

    def derive(self, center, extent, rel_sample_dist=0.05, rel_dense_sample_dist=0.025, calc_normal_relative=0.01):
        o = np.zeros(8)
        self.L.ptr_derive(_p(_f(center)), _p(_f(extent)), rel_sample_dist, rel_dense_sample_dist, calc_normal_relative, _p(o))
        return dict(diameter=o[0], r_min=o[1], dist_step=o[2], dist_step_dense=o[3], normal_r=o[4], view_pt=o[5:8].copy())

    def reference_indices(self, num, sample, seed):
        out = np.zeros(max(sample, 1), np.uint64)
        self.L.ptr_reference_indices(num, sample, seed, _p(out))
        return out[:sample].astype(np.int64)

    def prepare_model(self, points, normals, box=None, rel_sample_dist=0.05, rel_dense_sample_dist=0.025, calc_normal_relative=0.01,
                      invert_model_normal=False, keep_normals=False):
        """B1 - B6 without the two device calls: normals are the given or the estimated ones; -> dict(normals, sample_indices,
        dense_indices, info) -- the caller runs boundary detection on the dense sample"""
        xyz = _f(points)
        c, e = self.box(xyz) if box is None else (_f(box[0]), _f(box[1]))
        d = self.derive(c, e, rel_sample_dist, rel_dense_sample_dist, calc_normal_relative)
        nrm = _f(normals).copy()
        out, parent, info = np.zeros_like(xyz), np.zeros(len(xyz), np.int64), np.zeros(5, np.uint64)
        seed = self.L.ptr_prepare_normals(_p(xyz), _p(nrm), len(xyz), _p(d["view_pt"]), d["normal_r"], int(invert_model_normal),
                                          int(keep_normals), _p(out), _p(parent), _p(info))
        res = dict(normals=out, sample_indices=self.sample(xyz, d["dist_step"], seed),
                   dense_indices=self.sample(xyz, d["dist_step_dense"], seed) if rel_dense_sample_dist > 0 else np.zeros(0, np.int64))
        res["info"] = dict(d, box_center=c, box_extent=e, seed=int(seed), seed_flipped=int(info[0]), oriented=int(not keep_normals),
                           orient=dict(zip(STATS, (int(v) for v in info[1:]))))
        return res


STATS = ("rounds", "tree_edges", "component", "flips")


# ---- the judge: Kruskal under O2, then a breadth-first pass from the seed
def radius_edges(points, radius):
    """-> (d2, lo, hi) of every edge of rule O1, sorted by O2"""
    xyz = _f(points)
    r2 = radius * radius
    out = []
    for i in range(len(xyz)):
        d = xyz[i] - xyz[i + 1:]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        for j in np.nonzero(d2 < r2)[0]:
            out.append((float(d2[j]), i, i + 1 + int(j)))
    out.sort()
    return out


def judge_orient(points, normals, radius, seed):
    """-> (normals, parent, dict(tree_edges, component, flips), the tree's edge set)"""
    xyz, nrm = _f(points), _f(normals)
    n = len(xyz)
    root = list(range(n))

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x

    adj = [[] for _ in range(n)]
    tree = set()
    for _, lo, hi in radius_edges(xyz, radius):
        a, b = find(lo), find(hi)
        if a != b:
            root[a] = b
            adj[lo].append(hi)
            adj[hi].append(lo)
            tree.add((lo, hi))
    parent = np.full(n, -2, np.int64)
    sign = np.ones(n)
    out = nrm.copy()
    parent[seed] = -1
    queue, flips = [seed], 0
    for p in queue:
        for i in adj[p]:
            if parent[i] != -2:
                continue
            parent[i] = p
            dot = (nrm[i, 0] * nrm[p, 0] + nrm[i, 1] * nrm[p, 1]) + nrm[i, 2] * nrm[p, 2]
            if sign[p] * dot < 0:
                sign[i] = -1.0
                out[i] = -nrm[i]
                flips += 1
            queue.append(i)
    return out, parent, dict(tree_edges=len(tree), component=len(queue), flips=flips), tree


# ---- the input families of the orientation tests -> dict(points, normals, radius, seed)
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rand_normals(rng, n):
    return np.ascontiguousarray(_unit(rng.normal(size=(n, 3))) * rng.uniform(0.5, 2.0, size=(n, 1)))


def sphere_case(n, seed=5, radius=None):
    """points on the unit sphere, normals radial with random sign and length, the seed's outward"""
    rng = np.random.default_rng(seed)
    pts = _unit(rng.normal(size=(n, 3)))
    nrm = pts * rng.choice([-1.0, 1.0], size=(n, 1)) * rng.uniform(0.5, 2.0, size=(n, 1))
    nrm[0] = np.abs(nrm[0] / pts[0]) * pts[0]
    # ~ 20 neighbours on average: a cap of chord radius r holds n r^2 / 4 points
    r = radius if radius is not None else float(np.sqrt(4.0 * 20.0 / n))
    return dict(points=np.ascontiguousarray(pts + np.array([0.3, -0.2, 0.1])), normals=np.ascontiguousarray(nrm), radius=r, seed=0)


@functools.lru_cache(maxsize=None)
def orient_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "one":
        return dict(points=np.array([[0.1, 0.2, 0.3]]), normals=np.array([[0.0, 0.0, -1.0]]), radius=1.0, seed=0)
    if name == "two":
        return dict(points=np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]]), normals=np.array([[0.0, 0.0, 1.0], [0.0, 0.1, -1.0]]), radius=1.0, seed=1)
    if name.startswith("random_"):
        n = int(name[7:])
        return dict(points=rng.uniform(0, 1, size=(n, 3)), normals=_rand_normals(rng, n), radius=2.2 / n ** (1.0 / 3.0), seed=n // 2)
    if name == "path":
        n, r = 300, 0.01
        pts = np.zeros((n, 3))
        pts[:, 0] = np.cumsum(rng.uniform(0.85, 0.95, size=n)) * r       # spaced about 0.9 radius, no two gaps alike
        pts = pts[rng.permutation(n)]
        return dict(points=np.ascontiguousarray(pts), normals=_rand_normals(rng, n), radius=r, seed=7)
    if name == "lattice":
        g = np.stack(np.meshgrid(np.arange(8.0), np.arange(8.0), np.arange(8.0), indexing="ij"), axis=-1).reshape(-1, 3)
        g = g[rng.permutation(len(g))]
        return dict(points=np.ascontiguousarray(g), normals=_rand_normals(rng, len(g)), radius=1.5, seed=100)
    if name == "duplicates":
        pts = rng.uniform(0, 1, size=(400, 3))
        pts[380:] = pts[rng.integers(0, 380, size=20)]
        return dict(points=pts, normals=_rand_normals(rng, 400), radius=0.2, seed=390)
    if name == "two_clusters":
        pts = np.vstack([rng.uniform(0, 1, size=(150, 3)), rng.uniform(0, 1, size=(120, 3)) + np.array([3.0, 0, 0])])
        return dict(points=pts, normals=_rand_normals(rng, 270), radius=0.4, seed=10)
    if name == "on_radius":
        # 0 - 1 at exactly d2 == radius^2 (no edge), 1 - 2 and 2 - 3 inside: 0 is cut off
        pts = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.5, 0.25, 0.0], [0.5, 0.25, 0.375]])
        return dict(points=pts, normals=_rand_normals(rng, 4), radius=0.5, seed=2)
    if name == "full_cell":
        pts = np.vstack([rng.uniform(0.40, 0.45, size=(100, 3)), rng.uniform(0, 1, size=(300, 3))])   # > 64 points in one cell
        return dict(points=pts, normals=_rand_normals(rng, 400), radius=0.2, seed=3)
    if name == "zero_dots":
        pts = rng.uniform(0, 1, size=(300, 3))
        axes = np.eye(3)[rng.integers(0, 3, size=300)] * rng.choice([-1.0, 1.0], size=(300, 1))   # axis normals: dots are 0 or +-1
        return dict(points=pts, normals=np.ascontiguousarray(axes), radius=0.25, seed=0)
    if name == "sphere":
        return sphere_case(5000)
    raise KeyError(name)


ORIENT_CASES = ("one", "two", "random_255", "random_256", "random_257", "path", "lattice", "duplicates", "two_clusters", "on_radius",
                "full_cell", "zero_dots", "sphere")
TIE_FREE = ("random_255", "random_256", "random_257", "path", "two_clusters", "full_cell", "zero_dots")
