"""The plain-C restatement of the PPF voting contract in both modes (tests/cpp/ppf_ref.c) built into a temporary directory and
loaded with ctypes, an independent judge in numpy longdouble (acos / atan2 called directly, its own frame construction, no edge
tables), the input families and SampledPoints cases (the EdgePoints cases are in ppf_edge_ref_util), and what the GPU test files
of both modes ask of the library.  The mode is whether edge points are given: the model's to the table, the scene's to the vote."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
PI = np.arccos(LD(-1))
DEG = np.pi / 180.0
DEFAULTS = dict(rel_sample_dist=0.05, angle_step=12.0 * DEG, min_dist_thresh=1.0 / 3.0, min_angle_thresh=30.0 * DEG, faster_mode=True)
EDGE_BAND = 1e-9       # a quantity this close to a bin edge (rad; relative for the distance) leaves its pair undecided


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def sizes(diameter, p):
    angle_num = int(np.floor(np.pi / p["angle_step"] + 0.5)) + 1
    dist_num = int(np.floor(1.0 / p["rel_sample_dist"] + 0.5)) + 1
    return dict(angle_num=angle_num, alpha_num=2 * angle_num - 1, dist_num=dist_num, table_size=angle_num ** 3 * dist_num,
                dist_step=diameter * p["rel_sample_dist"])


# ---- ppf_ref.c
class RefModel:
    """a model of the restatement; edge_points / edge_normals make it an EdgePoints model (n_e > 0)"""

    def __init__(self, lib, points, normals, diameter, r_min, p, edge_points=None, edge_normals=None, centre_edges=True):
        self.L = lib
        self.n, self.n_e = len(points), 0 if edge_points is None else len(edge_points)
        ep, en = (None, None) if edge_points is None else (_f(edge_points), _f(edge_normals))
        self.h = lib.ppf_ref_create(_p(_f(points)), _p(_f(normals)), self.n, _p(ep), _p(en), self.n_e, float(diameter), float(r_min),
                                    p["rel_sample_dist"], p["angle_step"], p["min_dist_thresh"], p["min_angle_thresh"],
                                    int(bool(p["faster_mode"])), int(bool(centre_edges)))
        s = np.zeros(6, np.uint64)
        lib.ppf_ref_sizes(self.h, _p(s))
        self.table_size, self.n_entries, self.n_neighbors, self.angle_num, self.alpha_num, self.dist_num = (int(v) for v in s)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.ppf_ref_destroy(self.h)
            self.h = None

    def table(self):
        """-> dict(cell_offsets, entry_i, entry_alpha, nbr_offsets, nbr_indices, tmg, centroid)"""
        t = dict(cell_offsets=np.zeros(self.table_size + 1, np.uint32), entry_i=np.zeros(self.n_entries, np.uint16),
                 entry_alpha=np.zeros(self.n_entries, np.uint8), nbr_offsets=np.zeros(self.n + 1, np.uint32),
                 nbr_indices=np.zeros(self.n_neighbors, np.uint32), tmg=np.zeros((self.n, 4, 4)), centroid=np.zeros(3))
        self.L.ppf_ref_table(self.h, *(_p(t[k]) for k in ("cell_offsets", "entry_i", "entry_alpha", "nbr_offsets", "nbr_indices",
                                                          "tmg", "centroid")))
        return t

    def vote(self, scene_points, scene_normals, reference, edge_points=None, edge_normals=None):
        """edge_points / edge_normals: the scene's edge points (an EdgePoints model scans them, not the scene)
        -> dict(ref_pos, model_index, alpha_index, votes, poses, n_searched, visited, increments)"""
        sp, sn = _f(scene_points), _f(scene_normals)
        ep, en = (None, None) if edge_points is None else (_f(edge_points), _f(edge_normals))
        ref = np.ascontiguousarray(reference, dtype=np.uint64)
        cap = max(64, 8 * len(ref))
        while True:
            out = [np.zeros(cap, np.uint32) for _ in range(4)]
            poses = np.zeros((cap, 4, 4))
            searched = np.zeros(len(ref), np.uint32)
            st = np.zeros(2, np.uint64)
            k = self.L.ppf_ref_vote(self.h, _p(sp), _p(sn), len(sp), _p(ref), len(ref), _p(ep), _p(en), 0 if ep is None else len(ep), cap,
                                    *(_p(o) for o in out), _p(poses), _p(searched), _p(st))
            if k <= cap:
                break
            cap = k
        return dict(ref_pos=out[0][:k], model_index=out[1][:k], alpha_index=out[2][:k], votes=out[3][:k], poses=poses[:k],
                    n_searched=searched, visited=int(st[0]), increments=int(st[1]))

    def pair_bins(self, p0, n0, p1, n1, frame):
        q = np.zeros(4, np.int32)
        qa = C.c_int(0)
        ok = self.L.ppf_ref_pair_bins(self.h, _p(_f(p0)), _p(_f(n0)), _p(_f(p1)), _p(_f(n1)), _p(_f(frame).reshape(16)), _p(q),
                                      C.byref(qa))
        return (tuple(int(v) for v in q), qa.value) if ok else None

    def spread(self, q):
        cells = np.zeros(81, np.int64)
        k = self.L.ppf_ref_spread(self.h, _p(np.ascontiguousarray(q, dtype=np.int32)), _p(cells))
        return cells[:k]


class PpfRef:
    def __init__(self, tmpdir, openmp=False):
        so = os.path.join(str(tmpdir), "ppf_ref_omp.so" if openmp else "ppf_ref.so")
        if not os.path.exists(so):
            subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC"] + (["-fopenmp"] if openmp else []) +
                           [os.path.join(HERE, "cpp", "ppf_ref.c"), "-o", so, "-lm"], check=True)
        L = C.CDLL(so)
        L.ppf_ref_create.restype = C.c_void_p
        L.ppf_ref_create.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_double] * 6 + [C.c_int] * 2
        L.ppf_ref_destroy.argtypes = [C.c_void_p]
        L.ppf_ref_destroy.restype = None
        L.ppf_ref_sizes.argtypes = [C.c_void_p, C.c_void_p]
        L.ppf_ref_table.argtypes = [C.c_void_p] * 8
        L.ppf_ref_vote.restype = C.c_size_t
        L.ppf_ref_vote.argtypes = ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                    C.c_size_t, C.c_size_t] + [C.c_void_p] * 7)
        L.ppf_ref_edge_scores.restype = C.c_size_t
        L.ppf_ref_edge_scores.argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_uint64, C.c_double, C.c_int, C.c_void_p]
        L.ppf_ref_pair_bins.argtypes = [C.c_void_p] * 6 + [C.c_void_p, C.c_void_p]
        L.ppf_ref_spread.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ppf_ref_frame.argtypes = [C.c_void_p] * 3
        L.ppf_ref_frame.restype = None
        L.ppf_ref_local_maximum.restype = C.c_size_t
        L.ppf_ref_local_maximum.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        self.L = L

    def model(self, points, normals, diameter, r_min, p=None, edge_points=None, edge_normals=None, centre_edges=True):
        return RefModel(self.L, points, normals, diameter, r_min, p or params(), edge_points, edge_normals, centre_edges)

    def scores(self, votes, ratio, n_model, score_thresh, num_result):
        """E9: -> (the scores of votes sorted descending, the number kept)"""
        v = np.ascontiguousarray(votes, dtype=np.uint64)
        s = np.zeros(max(len(v), 1))
        keep = self.L.ppf_ref_edge_scores(_p(v), len(v), float(ratio), int(n_model), float(score_thresh), int(num_result), _p(s))
        return s[:len(v)], int(keep)

    def frame(self, p, n):
        T = np.zeros((4, 4))
        self.L.ppf_ref_frame(_p(_f(p)), _p(_f(n)), _p(T))
        return T

    def local_maximum(self, acc, vote_threshold, nbr_lists):
        """acc: rows x cols counts; nbr_lists: one index list per row -> [(row, column, votes)]"""
        acc = np.ascontiguousarray(acc, dtype=np.uint32)
        off = np.zeros(len(nbr_lists) + 1, np.uint32)
        off[1:] = np.cumsum([len(x) for x in nbr_lists])
        idx = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.uint32) for x in nbr_lists] + [np.zeros(0, np.uint32)]))
        out = np.zeros(3 * acc.shape[0] + 3, np.uint32)
        k = self.L.ppf_ref_local_maximum(_p(acc), acc.shape[0], acc.shape[1], int(vote_threshold), _p(off), _p(idx), _p(out))
        return [tuple(int(v) for v in out[3 * i:3 * i + 3]) for i in range(k)]


# ---- the judge: numpy longdouble, acos / atan2 directly
def judge_frame(p, n):
    """the rotation that turns n into +x about the axis (0, n_z, -n_y) (about +y when n is along x), as a rigid map that sends p
    to the origin: Rodrigues' formula, not the reference's quaternion"""
    p, n = np.asarray(p, dtype=LD), np.asarray(n, dtype=LD)
    u = np.array([LD(0), n[2], -n[1]])
    norm = np.sqrt(u[1] * u[1] + u[2] * u[2])
    u = u / norm if norm > 1e-6 else np.array([LD(0), LD(1), LD(0)])
    th = np.arccos(np.clip(n[0], LD(-1), LD(1)))
    K = np.array([[LD(0), -u[2], u[1]], [u[2], LD(0), -u[0]], [-u[1], u[0], LD(0)]])
    R = np.eye(3, dtype=LD) + np.sin(th) * K + (LD(1) - np.cos(th)) * (K @ K)
    T = np.eye(4, dtype=LD)
    T[:3, :3] = R
    T[:3, 3] = -(R @ p)
    return T


def _near_edge(x, step):
    """distance of x / step to the nearest half-integer, times step"""
    t = x / step
    return np.abs(t - (np.floor(t) + LD(0.5))) * step


def judge_pairs(p0, n0, T0, p1, n1, sz, p):
    """the bins of the pairs (p0, n0) -> (p1[j], n1[j]) under the frame T0 (longdouble 4 x 4): -> (valid, q (k, 4), qa, undecided)"""
    step = LD(p["angle_step"])
    p0, n0, p1, n1 = (np.asarray(a, dtype=LD) for a in (p0, n0, p1, n1))
    d = p1 - p0
    # the contract's d2 is the fp64 one: d2 == 0 is decided there
    d64 = np.asarray(p1, dtype=np.float64) - np.asarray(p0, dtype=np.float64)
    zero = ((d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1]) + d64[:, 2] * d64[:, 2]) == 0.0
    norm = np.sqrt((d * d).sum(axis=1))
    safe = np.where(zero, LD(1), norm)
    u = d / safe[:, None]
    f = np.stack([np.arccos(np.clip(u @ n0, -1, 1)), np.arccos(np.clip((u * n1).sum(axis=1), -1, 1)),
                  np.arccos(np.clip(n1 @ n0, -1, 1))], axis=1)
    q = np.floor(f / step + LD(0.5)).astype(np.int64)
    qd = np.floor(norm / LD(sz["dist_step"]) + LD(0.5)).astype(np.int64)
    t = p1 @ T0[:3, :3].T + T0[:3, 3]
    alpha = np.arctan2(-t[:, 2], t[:, 1])
    qa = np.floor((alpha + PI) / step + LD(0.5)).astype(np.int64)
    und = (_near_edge(f, step) < EDGE_BAND).any(axis=1) | (_near_edge(alpha + PI, step) < EDGE_BAND)
    und |= _near_edge(norm, LD(sz["dist_step"])) < EDGE_BAND * np.maximum(norm, LD(1e-300))
    valid = ~zero & (qd < sz["dist_num"])
    return valid, np.concatenate([q, qd[:, None]], axis=1), qa, und & ~zero


def judge_model(points, normals, diameter, r_min, p, edge_points=None, edge_normals=None, centre_edges=True):
    """M1 - M6, or E1 - E5 with the model's edge points -> dict like RefModel.table() + undecided (count) + points (centred,
    float64) + n_e (0 in SampledPoints mode)"""
    pts, nrm = _f(points), _f(normals)
    n = len(pts)
    sz = sizes(diameter, p)
    c = np.zeros(3)
    for i in range(n):
        c += pts[i]
    c /= float(n)
    cen = pts - c
    same = edge_points is None                  # the referred set is the sample: equal indices are no pairs
    rp, rn = (cen, nrm) if same else (_f(edge_points) - c if centre_edges else _f(edge_points).copy(), _f(edge_normals))
    n_r = len(rp)
    frames = [judge_frame(cen[i], nrm[i]) for i in range(n)]
    cells = np.full((n, n_r), sz["table_size"], np.int64)
    qas = np.zeros((n, n_r), np.int64)
    undecided = 0
    a = sz["angle_num"]
    for i in range(n):
        valid, q, qa, und = judge_pairs(cen[i], nrm[i], frames[i], rp, rn, sz, p)
        if same:
            valid[i] = False
            und[i] = False
        undecided += int(und.sum())
        cells[i] = np.where(valid, q[:, 0] + a * (q[:, 1] + a * (q[:, 2] + a * q[:, 3])), sz["table_size"])
        qas[i] = qa
    flat = cells.reshape(-1)
    order = np.argsort(flat, kind="stable")
    order = order[flat[order] < sz["table_size"]]
    off = np.zeros(sz["table_size"] + 1, np.uint32)
    off[1:] = np.cumsum(np.bincount(flat[order], minlength=sz["table_size"]))
    r = 0.5 * r_min
    nbr_off, nbr_idx = [0], []
    for i in range(n):
        dd = cen - cen[i]
        d2 = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
        nbr_idx.append(np.nonzero(d2 < r * r)[0])
        nbr_off.append(nbr_off[-1] + len(nbr_idx[-1]))
    return dict(cell_offsets=off, entry_i=(order // n_r).astype(np.uint16), entry_alpha=qas.reshape(-1)[order].astype(np.uint8),
                nbr_offsets=np.asarray(nbr_off, np.uint32), nbr_indices=np.concatenate(nbr_idx).astype(np.uint32),
                tmg=np.stack(frames), centroid=c, undecided=undecided, points=cen, normals=nrm, sizes=sz, n=n, n_e=0 if same else n_r)


def spread_cells(q, sz, k):
    """SpreadPPF -> the list of cells of one quantised feature"""
    a, out = sz["angle_num"], []
    for s0 in range(3):
        d = q[3] + s0 - 1
        if not 0 <= d < sz["dist_num"]:
            continue
        for s1 in range(k):
            a0 = q[0] + s1 - 1
            if not 0 <= a0 < a:
                continue
            for s2 in range(k):
                a1 = q[1] + s2 - 1
                if not 0 <= a1 < a:
                    continue
                for s3 in range(k):
                    a2 = q[2] + s3 - 1
                    if 0 <= a2 < a:
                        out.append(a0 + a * (a1 + a * (a2 + a * d)))
    return out


def local_maximum_py(acc, vote_threshold, nbr_lists):
    """CalcLocalMaximum in python -> [(row, column, votes)]"""
    acc = np.asarray(acc, dtype=np.int64)
    win = np.roll(acc, 1, axis=1) + acc + np.roll(acc, -1, axis=1)
    col = win.argmax(axis=1)                     # (the first maximum, columns ascending)
    best = win[np.arange(len(acc)), col]
    mx = int(best.max())
    if mx < vote_threshold:
        return []
    thr = int(float(mx) * 0.8)
    flag = np.ones(len(acc), bool)
    out = []
    for i in range(len(acc)):
        if not (best[i] > thr and flag[i]):
            continue
        is_max = True
        for j in nbr_lists[i]:
            if best[i] < best[j]:
                is_max = False
            else:
                flag[j] = False
        flag[i] = is_max
        if is_max:
            out.append((i, int(col[i]), int(best[i])))
    return out


def judge_pose(tsg, alpha_index, angle_step, tmg):
    """rule V8 in longdouble: tsg^-1 Rx(alpha index * angle_step) tmg -> float64"""
    al = LD(int(alpha_index)) * LD(angle_step)
    rx = np.eye(4, dtype=LD)
    rx[1, 1], rx[1, 2], rx[2, 1], rx[2, 2] = np.cos(al), -np.sin(al), np.sin(al), np.cos(al)
    inv = np.eye(4, dtype=LD)
    inv[:3, :3] = tsg[:3, :3].T
    inv[:3, 3] = -(tsg[:3, :3].T @ tsg[:3, 3])
    return (inv @ rx @ tmg).astype(np.float64)


def judge_vote(jm, r_min, p, scene_points, scene_normals, reference, edge_points=None, edge_normals=None):
    """the vote against a judge_model (V1 - V8; E6 - E8 with the scene's edge points, which are then the cloud that is scanned)
    -> dict(ref_pos, model_index, alpha_index, votes, poses, n_searched, undecided)"""
    rp, rn = _f(scene_points), _f(scene_normals)            # the reference points are read from the scene sample
    sp, sn = (rp, rn) if edge_points is None else (_f(edge_points), _f(edge_normals))
    sz, n = jm["sizes"], jm["n"]
    A, k = sz["alpha_num"], 2 if p["faster_mode"] else 3
    gate = int(float(jm["n_e"] or n) * 0.2)
    dist_thresh, cos_thresh = p["min_dist_thresh"] * r_min, np.cos(p["min_angle_thresh"])
    off, ei, ea = jm["cell_offsets"].astype(np.int64), jm["entry_i"].astype(np.int64), jm["entry_alpha"].astype(np.int64)
    nbrs = [jm["nbr_indices"][jm["nbr_offsets"][i]:jm["nbr_offsets"][i + 1]] for i in range(n)]
    res = dict(ref_pos=[], model_index=[], alpha_index=[], votes=[], poses=[], n_searched=[], undecided=0)
    for s, ri in enumerate(reference):
        p0, n0 = rp[ri], rn[ri]
        dd = sp - p0
        d2 = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
        near = d2 < r_min * r_min
        res["n_searched"].append(int(near.sum()))
        if not int(near.sum()) > gate:
            continue
        dots = (sn[:, 0] * n0[0] + sn[:, 1] * n0[1]) + sn[:, 2] * n0[2]
        keep = np.nonzero(near & ~((np.sqrt(d2) < dist_thresh) & (dots > cos_thresh)))[0]
        tsg = judge_frame(p0, n0)
        valid, q, qa, und = judge_pairs(p0, n0, tsg, sp[keep], sn[keep], sz, p)
        res["undecided"] += int(und.sum())
        seen = set()
        for t in np.nonzero(valid)[0]:
            for cell in spread_cells(q[t], sz, k):
                seen.add((cell, int(qa[t])))
        acc = np.zeros(n * A, np.int64)
        for cell, a in seen:
            e = slice(off[cell], off[cell + 1])
            np.add.at(acc, ei[e] * A + (ea[e] - a + A) % A, 1)
        for i, col, v in local_maximum_py(acc.reshape(n, A), gate, nbrs):
            res["ref_pos"].append(s)
            res["model_index"].append(i)
            res["alpha_index"].append(col)
            res["votes"].append(v)
            res["poses"].append(judge_pose(tsg, col, p["angle_step"], jm["tmg"][i]))
    return res


def judge_poses(c, ref_pos, model_index, alpha_index):
    """the poses tsg^-1 Rx(alpha index * angle_step) tmg of given maxima of case c, in longdouble with the judge's frames"""
    pts, nrm = _f(c["points"]), _f(c["normals"])
    cen = np.zeros(3)
    for i in range(len(pts)):
        cen += pts[i]
    cen /= float(len(pts))
    out = []
    for s, i, col in zip(ref_pos, model_index, alpha_index):
        ri = int(c["reference"][int(s)])
        tsg = judge_frame(c["scene_points"][ri], c["scene_normals"][ri])
        tmg = judge_frame(pts[int(i)] - cen, nrm[int(i)])
        out.append(judge_pose(tsg, col, c["params"]["angle_step"], tmg))
    return np.asarray(out).reshape(-1, 4, 4)


# ---- the input families
def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _tilt_frame(rng):
    """an orthonormal basis (a, b, normal) and a unit vector tilted a few degrees off the normal"""
    nrm = _unit(rng.normal(size=3))
    a = _unit(np.cross(nrm, [1.0, 0.0, 0.0] if abs(nrm[0]) < 0.9 else [0.0, 1.0, 0.0]))
    b = np.cross(nrm, a)
    # (the tilt's two components have no small-integer ratio: no lattice direction of the grid is perpendicular to it)
    return a, b, nrm, _unit(nrm + 0.1137 * a + 0.0619 * b)


def family(name, n, seed):
    """-> (points (n, 3), unit normals (n, 3), diameter).  The plate's and the grid's normals are tilted a few degrees off the
    plane's and the box's carry a small noise: a normal exactly perpendicular to every in-plane difference puts f0 = f1 = pi / 2
    on a bin edge of the 12 degree step."""
    rng = np.random.default_rng(seed)
    if name == "random":
        pts, nrm = rng.uniform(-0.5, 0.5, size=(n, 3)), _unit(rng.normal(size=(n, 3)))
    elif name == "sphere":
        nrm = _unit(rng.normal(size=(n, 3)))
        pts = 0.5 * nrm + np.array([0.3, -0.2, 0.1])
    elif name == "box":
        face = rng.integers(0, 6, size=n)
        pts = rng.uniform(-0.5, 0.5, size=(n, 3)) * np.array([1.0, 0.7, 0.4])
        nrm = np.zeros((n, 3))
        half = 0.5 * np.array([1.0, 0.7, 0.4])
        for i in range(n):
            ax, sg = face[i] // 2, 1.0 if face[i] % 2 else -1.0
            pts[i, ax] = sg * half[ax]
            nrm[i, ax] = sg
        nrm = _unit(nrm + rng.normal(0, 0.02, size=(n, 3)))
    elif name == "plate":
        a, b, _, tilted = _tilt_frame(rng)
        uv = rng.uniform(-0.5, 0.5, size=(n, 2))
        pts = uv[:, :1] * a + uv[:, 1:] * b
        nrm = np.tile(tilted, (n, 1))
    elif name == "grid":
        a, b, _, tilted = _tilt_frame(rng)
        side = int(np.ceil(np.sqrt(n)))
        ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2)[:n].astype(np.float64)
        h = 0.97 / side
        pts = (ij[:, :1] * h - 0.45) * a + (ij[:, 1:] * h - 0.45) * b
        nrm = np.tile(tilted, (n, 1))
    else:
        raise KeyError(name)
    ext = pts.max(axis=0) - pts.min(axis=0)
    return np.ascontiguousarray(pts), np.ascontiguousarray(nrm), float(np.linalg.norm(ext))


FAMILIES = ("random", "sphere", "box", "plate", "grid")


def pose(seed):
    rng = np.random.default_rng(1000 + seed)
    ax = _unit(rng.normal(size=3))
    th = rng.uniform(0.3, 2.5)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = rng.uniform(-0.4, 0.4, size=3)
    return T


def scene_of(points, normals, T, n_clutter, seed):
    """the posed copy of a cloud, then clutter around it, shuffled -> (points, normals, indices of the copy's points)"""
    rng = np.random.default_rng(2000 + seed)
    sp = points @ T[:3, :3].T + T[:3, 3]
    sn = normals @ T[:3, :3].T
    lo, hi = sp.min(axis=0) - 0.3, sp.max(axis=0) + 0.3
    cp = rng.uniform(lo, hi, size=(n_clutter, 3))
    cn = _unit(rng.normal(size=(n_clutter, 3)))
    allp, alln = np.vstack([sp, cp]), np.vstack([sn, cn])
    perm = rng.permutation(len(allp))
    where = np.empty(len(allp), np.int64)
    where[perm] = np.arange(len(allp))
    return np.ascontiguousarray(allp[perm]), np.ascontiguousarray(alln[perm]), where[:len(points)]


def counted_scene(points, normals, T, r_min, count, seed):
    """a scene whose reference point 0 has exactly `count` neighbours within r_min (itself included): the posed copy's points
    nearest to its first one, and the copy's points beyond 1.05 r_min"""
    sp = points @ T[:3, :3].T + T[:3, 3]
    sn = normals @ T[:3, :3].T
    d = np.linalg.norm(sp - sp[0], axis=1)
    order = np.argsort(d, kind="stable")
    inside = order[d[order] < 0.999 * r_min]
    assert len(inside) >= count, (len(inside), count)
    keep = np.concatenate([inside[:count], np.nonzero(d > 1.05 * r_min)[0]])
    assert keep[0] == 0
    return np.ascontiguousarray(sp[keep]), np.ascontiguousarray(sn[keep])


# ---- the cases of the GPU tests (tests/test_ppf.py holds ppf_ref.c to the judge on every one of them)
TABLE_SIZES = (2, 3, 63, 64, 65, 255, 256, 257)
TABLE_LARGE = 1500
TABLE_LARGE_SEED = 21    # (a seed whose 2 248 500 pairs are all decided)
VOTE_N = 320            # the model of the vote cases: the gate is size_t(0.2 n) = 64 neighbours
ANGLE_STEPS = {"12": 12.0 * DEG, "11.25": 11.25 * DEG, "6": 6.0 * DEG}
LDS_EDGE_N = 1175       # the largest model of the LDS path at 61 bins (6 degrees); 1176 is in device memory


@functools.lru_cache(maxsize=None)
def model_case(name, n=VOTE_N, seed=None):
    seeds = {"random": 11, "sphere": 12, "box": 13, "plate": 14, "grid": 15}
    pts, nrm, diameter = family(name, n, seeds[name] if seed is None else seed)
    return pts, nrm, diameter, 0.45 * diameter    # r_min


@functools.lru_cache(maxsize=None)
def vote_case(name, n=VOTE_N, n_ref=12, clutter=400):
    """-> (model points, normals, diameter, r_min, scene points, scene normals, reference indices, true pose)"""
    pts, nrm, diameter, r_min = model_case(name, n)
    T = pose(len(name))
    sp, sn, where = scene_of(pts, nrm, T, clutter, len(name))
    ref = np.sort(where[:: max(1, n // n_ref)][:n_ref])
    return pts, nrm, diameter, r_min, sp, sn, ref, T


def _case(model, p, scene, ref):
    pts, nrm, diameter, r_min = model
    return dict(points=pts, normals=nrm, diameter=diameter, r_min=r_min, params=p, scene_points=scene[0], scene_normals=scene[1],
                reference=np.asarray(ref, dtype=np.int64))


COUNTS = (63, 64, 65, 255, 256, 257)     # neighbours of the one reference point; 64 = size_t(0.2 * 320): no vote, 65: the first vote
VOTE_CASES = (tuple("family_" + f for f in FAMILIES) + ("step_11.25", "step_6", "full_spread", "full_spread_6") +
              tuple("count_%s_%d" % (f, c) for f in FAMILIES for c in COUNTS) + ("one_ref", "duplicate_ref", "beyond_dist_num", "lds_edge", "lds_edge_plus_1"))


@functools.lru_cache(maxsize=None)
def case(name):
    """the inputs of one vote case of tests/test_gpu_ppf.py -> dict(points, normals, diameter, r_min, params, scene_points,
    scene_normals, reference)"""
    if name.startswith("family_"):
        pts, nrm, diameter, r_min, sp, sn, ref, _ = vote_case(name[7:])
        return _case((pts, nrm, diameter, r_min), params(), (sp, sn), ref)
    if name in ("step_11.25", "step_6", "full_spread", "full_spread_6"):
        fam = {"step_11.25": "box", "step_6": "sphere", "full_spread": "random", "full_spread_6": "box"}[name]
        step = {"step_11.25": "11.25", "step_6": "6", "full_spread": "12", "full_spread_6": "6"}[name]
        pts, nrm, diameter, r_min, sp, sn, ref, _ = vote_case(fam, n_ref=6)
        return _case((pts, nrm, diameter, r_min), params(angle_step=ANGLE_STEPS[step], faster_mode=not name.startswith("full")),
                     (sp, sn), ref)
    if name.startswith("count_"):
        _, fam, count = name.split("_")
        pts, nrm, diameter, _ = model_case(fam)
        r_min = 1.2 * diameter            # every model point is a neighbour of every other
        # (the plate's and the grid's normals are parallel: the pair filter would drop every near neighbour at the default
        # distance threshold)
        return _case((pts, nrm, diameter, r_min), params(min_dist_thresh=0.01), counted_scene(pts, nrm, pose(5), r_min, int(count), 5), [0])
    if name == "one_ref":
        pts, nrm, diameter, r_min, sp, sn, ref, _ = vote_case("box")
        return _case((pts, nrm, diameter, r_min), params(), (sp, sn), ref[3:4])
    if name == "duplicate_ref":
        # every reference point once more at the end of the scene, its normal turned: pairs with d2 == 0 that pass the filter
        pts, nrm, diameter, r_min, sp, sn, ref, _ = vote_case("sphere")
        R = pose(77)[:3, :3]
        return _case((pts, nrm, diameter, r_min), params(), (np.vstack([sp, sp[ref]]), np.vstack([sn, sn[ref] @ R.T])), ref)
    if name == "beyond_dist_num":
        # a stated diameter of 0.6 of the true one: model and scene pairs whose quantised distance is >= dist_num
        pts, nrm, diameter, r_min, sp, sn, ref, _ = vote_case("random")
        return _case((pts, nrm, 0.6 * diameter, r_min), params(), (sp, sn), ref)
    if name in ("lds_edge", "lds_edge_plus_1"):
        n = LDS_EDGE_N + (name != "lds_edge")
        pts, nrm, diameter, r_min, sp, sn, ref, _ = vote_case("box", n=n, n_ref=4, clutter=300)
        return _case((pts, nrm, diameter, r_min), params(angle_step=ANGLE_STEPS["6"]), (sp, sn), ref)
    raise KeyError(name)


# ---- a case through the restatement and through the library.  A case dict with edge_points / edge_normals and scene_edge_points /
# scene_edge_normals (ppf_edge_ref_util) is an EdgePoints case; without them it is a SampledPoints case
INTS = ("ref_pos", "model_index", "alpha_index", "votes")
TABLE = ("cell_offsets", "entry_i", "entry_alpha", "nbr_offsets", "nbr_indices")

# the SampledPoints cases that tests/test_ppf_edge.py also runs as EdgePoints cases on themselves
OWN_EDGE_CASES = ("family_box", "family_plate", "count_grid_65", "count_random_64", "step_6", "full_spread", "lds_edge_plus_1")


def with_own_edges(c):
    """the SampledPoints case c as an EdgePoints case: the sample is its own edge set, the scene its own edge cloud"""
    return dict(c, edge_points=c["points"], edge_normals=c["normals"], scene_edge_points=c["scene_points"],
                scene_edge_normals=c["scene_normals"])


def ref_model(ref, c, **kw):
    return ref.model(c["points"], c["normals"], c["diameter"], c["r_min"], c["params"], c.get("edge_points"), c.get("edge_normals"), **kw)


def ref_vote(m, c):
    return m.vote(c["scene_points"], c["scene_normals"], c["reference"], c.get("scene_edge_points"), c.get("scene_edge_normals"))


def lib_model(capi, c):
    p = c["params"]
    return capi.PpfModel(c["points"], c["normals"], c["diameter"], c["r_min"], edge_points=c.get("edge_points"),
                         edge_normals=c.get("edge_normals"), rel_sample_dist=p["rel_sample_dist"], angle_step=p["angle_step"],
                         min_dist_thresh=p["min_dist_thresh"], min_angle_thresh=p["min_angle_thresh"], faster_mode=p["faster_mode"])


def lib_vote(m, c, **kw):
    return m.vote(c["scene_points"], c["scene_normals"], c["reference"], edge_points=c.get("scene_edge_points"),
                  edge_normals=c.get("scene_edge_normals"), **kw)


def forced_vote(capi, c, device_memory=False, max_groups=0, model=None):
    """the vote with its accumulators forced into device memory and / or its workgroups capped -> (model, (result, stats))"""
    capi.ppf_force(device_memory, max_groups)
    try:
        m = model or lib_model(capi, c)
        return m, lib_vote(m, c, stats=True)
    finally:
        capi.ppf_force(False, 0)


def assert_table(t, want):
    for k in TABLE:
        assert np.array_equal(t[k], want[k]), k
    assert np.array_equal(t["centroid"], want["centroid"])
    assert np.abs(t["tmg"] - want["tmg"]).max() < 1e-12      # (host arithmetic on both sides)


def assert_vote(c, got, stats, want):
    for k in INTS:
        assert np.array_equal(got[k], want[k]), k
    assert stats["neighbours_visited"] == want["visited"] and stats["increments"] == want["increments"]
    if len(want["votes"]):
        assert np.abs(got["poses"] - judge_poses(c, got["ref_pos"], got["model_index"], got["alpha_index"])).max() < 1e-12
