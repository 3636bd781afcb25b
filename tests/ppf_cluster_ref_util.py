"""The plain-C restatement of the PPF pose clustering contract (tests/cpp/ppf_cluster_ref.c, K1 - K6 and K8) built into a temporary
directory and loaded with ctypes; K7 put together from the ICP restatements (icp_ref_util, icp_l1_ref_util); an independent judge
in numpy longdouble (arccos called directly, numpy.linalg.eigh for the average); a line-by-line simulation of the reference's
GatherPose with its stack; and the input families both test files use."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
DEG = np.pi / 180.0
R_DIST = 0.05                # dist_threshold of every family (a model of diameter 1)
ANGLE = 12.0 * DEG           # angle_threshold of every family
BAND = 1e-9                  # a pair this close to a threshold (relative for the distance, rad for the angle) is undecided


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# ---- ppf_cluster_ref.c
class PcRef:
    def __init__(self, tmpdir, openmp=False):
        so = os.path.join(str(tmpdir), "ppf_cluster_ref_omp.so" if openmp else "ppf_cluster_ref.so")
        if not os.path.exists(so):
            subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC"] + (["-fopenmp"] if openmp else []) +
                           [os.path.join(HERE, "cpp", "ppf_cluster_ref.c"), "-o", so, "-lm"], check=True)
        L = C.CDLL(so)
        L.pcr_threshold.restype = C.c_size_t
        L.pcr_threshold.argtypes = [C.c_uint32]
        L.pcr_cluster.restype = C.c_size_t
        L.pcr_cluster.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_double] + [C.c_void_p] * 12
        L.pcr_finish.restype = C.c_size_t
        L.pcr_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_double, C.c_uint64, C.c_double, C.c_int] + [C.c_void_p] * 3
        for fn in (L.pcr_mat_to_quat, L.pcr_quat_to_mat):
            fn.restype, fn.argtypes = None, [C.c_void_p, C.c_void_p]
        L.pcr_jacobi4.restype, L.pcr_jacobi4.argtypes = None, [C.c_void_p] * 3
        L.pcr_average.restype, L.pcr_average.argtypes = None, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.pcr_match.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int]
        self.L = L

    def threshold(self, max_votes):
        return int(self.L.pcr_threshold(int(max_votes)))

    def cluster(self, poses, votes, dist_threshold=R_DIST, angle_threshold=ANGLE):
        """-> the dict capi.ppf_cluster_poses returns (without stats' timings): K1 - K6"""
        T = _f(poses).reshape(-1, 4, 4)
        v = np.ascontiguousarray(votes, dtype=np.uint32).reshape(-1)
        P = max(len(T), 1)
        u32 = [np.zeros(P, np.uint32) for _ in range(3)]      # order, count_t, count_r
        i32 = [np.full(P, -1, np.int32) for _ in range(3)]    # label_t, label_r, min_num_pt_r
        min_t = C.c_int32(0)
        cvotes, avotes, acl, avg = np.zeros(P, np.uint64), np.zeros(P, np.uint64), np.zeros(P, np.uint32), np.zeros((P, 4, 4))
        counts = np.zeros(2, np.uint64)
        n = self.L.pcr_cluster(_p(T), _p(v), len(T), float(dist_threshold), float(angle_threshold), _p(u32[0]), _p(u32[1]), _p(i32[0]),
                               _p(u32[2]), _p(i32[1]), C.cast(C.byref(min_t), C.c_void_p), _p(i32[2]), _p(cvotes), _p(avg), _p(avotes),
                               _p(acl), _p(counts))
        ct, cr = int(counts[0]), int(counts[1])
        return dict(order=u32[0][:n], count_t=u32[1][:n], label_t=i32[0][:n], count_r=u32[2][:n], label_r=i32[1][:n],
                    min_num_pt_t=int(min_t.value), min_num_pt_r=i32[2][:ct], cluster_votes=cvotes[:ct], avg_poses=avg[:cr],
                    avg_votes=avotes[:cr], avg_cluster=acl[:cr],
                    stats=dict(n_valid=n, clusters_t=ct, clusters_r=cr, pair_tests=6 * n * n))

    def finish(self, poses, votes, centroid, ratio, n_model, score_thresh, num_result):
        """K8 -> dict(poses, q, t, votes, scores)"""
        T = _f(poses).reshape(-1, 4, 4).copy()
        v = np.ascontiguousarray(votes, dtype=np.uint64).reshape(-1).copy()
        k = len(v)
        q, t, s = np.zeros((max(k, 1), 4)), np.zeros((max(k, 1), 3)), np.zeros(max(k, 1))
        keep = self.L.pcr_finish(_p(T), _p(v), k, _p(_f(centroid)), float(ratio), int(n_model), float(score_thresh), int(num_result),
                                 _p(q), _p(t), _p(s))
        return dict(poses=T[:keep], q=q[:keep], t=t[:keep], votes=v[:keep], scores=s[:keep])

    def mat_to_quat(self, R):
        q = np.zeros(4)
        self.L.pcr_mat_to_quat(_p(_f(R).reshape(9)), _p(q))
        return q

    def quat_to_mat(self, q):
        R = np.zeros((3, 3))
        self.L.pcr_quat_to_mat(_p(_f(q)), _p(R))
        return R

    def jacobi4(self, A):
        w, V = np.zeros(4), np.zeros((4, 4))
        self.L.pcr_jacobi4(_p(_f(A).reshape(16)), _p(w), _p(V))
        return w, V

    def average(self, poses, votes):
        """-> (the 4 x 4 sum of q q^T, the sum of t, the averaged pose)"""
        T = _f(poses).reshape(-1, 4, 4)
        s, out = np.zeros(13), np.zeros((4, 4))
        self.L.pcr_average(_p(T), _p(np.ascontiguousarray(votes, dtype=np.uint32)), len(T), _p(s), _p(out))
        M = np.zeros((4, 4))
        M[np.triu_indices(4)] = s[:10]
        return M + np.triu(M, 1).T, s[10:], out

    def match(self, a, b, level, dist_threshold=R_DIST, angle_threshold=ANGLE):
        return bool(self.L.pcr_match(_p(_f(a).reshape(16)), _p(_f(b).reshape(16)), float(dist_threshold), float(angle_threshold), int(level)))


def estimate_ref(pc, icp, raw_poses, raw_votes, model_centred, centroid, scene_points, scene_normals, dist_step, dist_threshold,
                 angle_threshold=ANGLE, ratio=0.6, score_thresh=0.6, rel_dist_sparse_thresh=5.0, num_result=10, refine_method="PointToPlane"):
    """K1 - K8 from the raw poses of a vote: pc a PcRef (K1 - K6, K8), icp an icp_ref_util.IcpRef (K7: its point-to-point
    loop, or icp_l1_ref_util's L1 loop over its search).  -> PcRef.finish's dict + `clusters` (K1 - K6) + `refined` (K7's
    poses in translation-cluster order, before the shift)"""
    import icp_l1_ref_util as l1

    cl = pc.cluster(raw_poses, raw_votes, dist_threshold, angle_threshold)
    picked, votes = [], []
    for t in range(len(cl["cluster_votes"])):
        sub = np.nonzero(cl["avg_cluster"] == t)[0]
        if len(sub) == 0:
            continue
        best = sub[int(np.argmax(cl["avg_votes"][sub]))]       # (the first maximum: std::max_element)
        T = cl["avg_poses"][best]
        max_dist = rel_dist_sparse_thresh * dist_step
        if refine_method == "PointToPoint":
            T = icp.icp(model_centred, scene_points, max_dist, init=T, max_iteration=30)["T"]
        elif refine_method == "PointToPlane":
            T = l1.icp_l1(icp, model_centred, scene_points, max_dist, T, 30, scene_normals)["T"]
        picked.append(np.asarray(T).reshape(4, 4))
        votes.append(int(cl["avg_votes"][best]))
    res = pc.finish(np.asarray(picked).reshape(-1, 4, 4), votes, centroid, ratio, len(model_centred), score_thresh, num_result)
    res["clusters"], res["refined"] = cl, np.asarray(picked).reshape(-1, 4, 4)
    return res


# ---- the judge: numpy longdouble, arccos directly, eigh
def _min_num_pt(counts):
    return int(max(6, int(counts.max()) if len(counts) else 0) / 2.0)


def _gather(adj, votes, members):
    """K4 over `members` (ascending positions) with their boolean match matrix -> (counts, rank per member (-1 dropped), min_num_pt,
    cluster votes in rank order).  Components by min-label propagation over the cores."""
    k = len(members)
    counts = adj.sum(axis=1).astype(np.int64)
    min_pt = _min_num_pt(counts)
    core = counts >= min_pt
    big = k + 1
    lab = np.where(core, np.arange(k), big)
    cc = adj & core[None, :] & core[:, None]
    while True:
        new = np.where(core, np.where(cc, lab[None, :], big).min(axis=1, initial=big), big)
        new = np.minimum(new, lab)
        if np.array_equal(new, lab):
            break
        lab = new
    border = np.where(adj & core[None, :], lab[None, :], big).min(axis=1, initial=big)
    lab = np.where(core, lab, border)
    roots = [r for r in np.unique(lab) if r != big]
    info = []
    for r in roots:
        mem = np.nonzero(lab == r)[0]
        info.append((-int(votes[members[mem]].sum()), int(members[mem].min()), int(r)))
    info.sort()
    rank_of = {r: i for i, (_, _, r) in enumerate(info)}
    rank = np.array([rank_of.get(int(x), -1) for x in lab], dtype=np.int64)
    return counts, rank, min_pt, np.array([-v for v, _, _ in info], dtype=np.uint64)


def _quat_ld(R):
    """a unit quaternion of a rotation, by the largest of (w, x, y, z): not MatToQuat's branches"""
    R = np.asarray(R, dtype=LD)
    d = np.array([R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], -R[0, 0] + R[1, 1] - R[2, 2], -R[0, 0] - R[1, 1] + R[2, 2]])
    k = int(np.argmax(d))
    h = np.sqrt(LD(1) + d[k]) / 2
    if k == 0:
        q = [h, (R[2, 1] - R[1, 2]) / (4 * h), (R[0, 2] - R[2, 0]) / (4 * h), (R[1, 0] - R[0, 1]) / (4 * h)]
    elif k == 1:
        q = [(R[2, 1] - R[1, 2]) / (4 * h), h, (R[0, 1] + R[1, 0]) / (4 * h), (R[0, 2] + R[2, 0]) / (4 * h)]
    elif k == 2:
        q = [(R[0, 2] - R[2, 0]) / (4 * h), (R[0, 1] + R[1, 0]) / (4 * h), h, (R[1, 2] + R[2, 1]) / (4 * h)]
    else:
        q = [(R[1, 0] - R[0, 1]) / (4 * h), (R[0, 2] + R[2, 0]) / (4 * h), (R[1, 2] + R[2, 1]) / (4 * h), h]
    return np.array(q, dtype=LD)


def _average(poses):
    """-> (averaged pose float64, eigenvalues ascending)"""
    M = np.zeros((4, 4), dtype=LD)
    for T in poses:
        q = _quat_ld(T[:3, :3])
        M += np.outer(q, q)
    w, V = np.linalg.eigh(M.astype(np.float64))
    q = V[:, 3].astype(LD)
    if q[int(np.argmax(np.abs(q)))] < 0:
        q = -q
    a, b, c, d = q
    R = np.array([[1 - 2 * (c * c + d * d), 2 * (b * c - a * d), 2 * (a * c + b * d)],
                  [2 * (b * c + a * d), 1 - 2 * (b * b + d * d), 2 * (c * d - a * b)],
                  [2 * (b * d - a * c), 2 * (a * b + c * d), 1 - 2 * (b * b + c * c)]], dtype=LD)
    out = np.eye(4)
    out[:3, :3] = R.astype(np.float64)
    out[:3, 3] = (np.asarray(poses, dtype=LD)[:, :3, 3].sum(axis=0) / LD(len(poses))).astype(np.float64)
    return out, w


def judge(poses, votes, dist_threshold=R_DIST, angle_threshold=ANGLE):
    """K1 - K6 decided in longdouble -> the dict of PcRef.cluster + undecided (pairs within BAND of a threshold), eigen_gaps
    ((l4 - l3) / count per sub-cluster), adj_t / adj_r (the match matrices over the valid poses), bridges (non-core poses with core
    neighbours in two translation clusters)"""
    T = _f(poses).reshape(-1, 4, 4)
    v = np.asarray(votes, dtype=np.int64).reshape(-1)
    P = len(T)
    order = np.array(sorted(range(P), key=lambda i: (-int(v[i]), i)), dtype=np.int64)
    thr = int(float(v[order[0]]) * 0.5) if P else 0
    n = int((v[order] >= thr).sum()) if P else 0      # (the prefix: the votes descend)
    order = order[:n]
    S, sv = T[order], v[order]
    t = S[:, :3, 3].astype(LD)
    d = t[:, None, :] - t[None, :, :]
    dist = np.sqrt((d * d).sum(axis=2))
    r = LD(dist_threshold)
    adj_t = dist < r
    R = S[:, :3, :3].astype(LD)
    ca = (np.einsum("iab,jab->ij", R, R) - LD(1)) / LD(2)
    ang = np.arccos(np.clip(ca, LD(-1), LD(1)))
    adj_r = adj_t & (ang < LD(angle_threshold))
    off = ~np.eye(n, dtype=bool)
    undecided = int(((np.abs(dist - r) < LD(BAND) * r) & off).sum() + ((np.abs(ang - LD(angle_threshold)) < LD(BAND)) & off).sum()) // 2
    members = np.arange(n)
    count_t, label_t, min_t, cvotes = _gather(adj_t, sv, members)
    count_r, label_r = np.zeros(n, np.int64), np.full(n, -1, np.int64)
    min_r, avg, avotes, acl, gaps = [], [], [], [], []
    for c in range(len(cvotes)):
        mem = np.nonzero(label_t == c)[0]
        cnt, rk, mp, sub_votes = _gather(adj_r[np.ix_(mem, mem)], sv, mem)
        count_r[mem], label_r[mem] = cnt, rk
        min_r.append(mp)
        for s in range(len(sub_votes)):
            who = mem[rk == s]
            pose, w = _average(S[who])
            avg.append(pose)
            avotes.append(int(sub_votes[s]))
            acl.append(c)
            gaps.append(float((w[3] - w[2]) / len(who)))
    core = count_t >= min_t
    bridges = [int(i) for i in range(n) if not core[i] and len(set(label_t[np.nonzero(adj_t[i] & core)[0]])) >= 2]
    return dict(order=order.astype(np.uint32), count_t=count_t.astype(np.uint32), label_t=label_t.astype(np.int32),
                count_r=count_r.astype(np.uint32), label_r=label_r.astype(np.int32), min_num_pt_t=min_t,
                min_num_pt_r=np.asarray(min_r, dtype=np.int32), cluster_votes=cvotes, avg_poses=np.asarray(avg).reshape(-1, 4, 4),
                avg_votes=np.asarray(avotes, dtype=np.uint64), avg_cluster=np.asarray(acl, dtype=np.uint32),
                stats=dict(n_valid=n, clusters_t=len(cvotes), clusters_r=len(avg), pair_tests=6 * n * n),
                undecided=undecided, eigen_gaps=gaps, adj_t=adj_t, adj_r=adj_r, dist=dist.astype(np.float64), bridges=bridges)


INT_KEYS = ("order", "count_t", "label_t", "count_r", "label_r", "min_num_pt_r", "cluster_votes", "avg_votes", "avg_cluster")


def assert_same_integers(a, b, stats=True):
    """every integer of two results of K1 - K6"""
    for k in INT_KEYS:
        assert np.array_equal(np.asarray(a[k]).astype(np.int64), np.asarray(b[k]).astype(np.int64)), k
    assert int(a["min_num_pt_t"]) == int(b["min_num_pt_t"])
    if stats:
        for k in ("n_valid", "clusters_t", "clusters_r", "pair_tests"):
            assert int(a["stats"][k]) == int(b["stats"][k]), k


# ---- the reference's GatherPose, line by line (src/ppf_estimation.cpp:778-836), over the valid poses
def simulate_gather(neighbours, votes):
    """neighbours[ci]: the neighbour list of pose ci as the reference holds it (level 1: the kd-tree's radius search, ascending
    distance, itself first) -> the clusters as lists of pose indices in arrival order, sorted by votes descending"""
    n_pose = len(neighbours)
    if n_pose == 0:
        return []
    min_num_pt = 6
    for i in range(n_pose):
        num = len(neighbours[i])
        if num > min_num_pt:
            min_num_pt = num
    min_num_pt = int(min_num_pt / 2.0)
    check = [False] * n_pose
    clusters = []
    for pi in range(n_pose):
        ci = pi
        if check[ci] or len(neighbours[ci]) < min_num_pt:
            continue
        members, total = [], 0
        stack = [ci]
        while stack:
            ci = stack.pop()
            if check[ci]:
                continue
            members.append(ci)
            total += int(votes[ci])
            check[ci] = True
            for ni in neighbours[ci]:
                if check[ni]:
                    continue
                if len(neighbours[ni]) >= min_num_pt:
                    stack.append(ni)
                else:
                    members.append(ni)
                    total += int(votes[ni])
                    check[ni] = True
        clusters.append((total, members))
    clusters.sort(key=lambda c: -c[0])     # (stable; std::sort leaves ties open)
    return clusters


def reference_level1(j, votes):
    """the reference's level-1 clusters of a judged input (votes: the caller's, by input index): the kd-tree's radius search per
    valid pose, then GatherPose -> the set of member sets (sorted positions)"""
    n = len(j["order"])
    nbrs = []
    for i in range(n):
        who = np.nonzero(j["adj_t"][i])[0]
        nbrs.append([int(x) for x in who[np.argsort(j["dist"][i][who], kind="stable")]])
    sv = np.asarray(votes)[j["order"].astype(np.int64)]
    return {frozenset(m) for _, m in simulate_gather(nbrs, sv)}


def member_sets(labels):
    """the clusters of a label array as a set of member sets"""
    labels = np.asarray(labels)
    return {frozenset(int(x) for x in np.nonzero(labels == c)[0]) for c in np.unique(labels) if c >= 0}


# ---- the input families (fixed seeds; rotations from axis-angle, votes small integers)
def rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def _ball(rng, radius):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v) * radius * rng.uniform(0.0, 1.0) ** (1 / 3)


def _jitter(rng, R, max_deg=3.0):
    return R @ rot(rng.normal(size=3), rng.uniform(0.0, max_deg) * DEG)


BLOB_SIZES = (2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2049)


def _blobs(P, seed, distinct=False):
    """k pose clusters, a fringe around each, a blob too small to be one, and low-vote clutter"""
    rng = np.random.default_rng(seed)
    r = R_DIST
    poses, votes = [], []
    n_clutter = P // 4
    n_in = P - n_clutter
    if n_in >= 40:
        tiny = 3
        rest = n_in - tiny
        sizes = [rest - rest // 3 - rest // 4, rest // 3, rest // 4, tiny]
    else:
        sizes = [n_in]
    for b, size in enumerate(sizes):
        centre = np.array([0.6 * b - 0.9, 0.35 * ((b * 7) % 3 - 1), 0.2 * b])
        Rb = rot(rng.normal(size=3), rng.uniform(0.2, 2.8))
        Rb2 = Rb @ rot([0.3, -1.0, 0.5], 40.0 * DEG)
        n_fringe = size // 8 if size >= 16 else 0
        for m in range(size):
            if m < size - n_fringe:
                t = centre + _ball(rng, 0.3 * r)
            else:
                d = rng.normal(size=3)
                t = centre + d / np.linalg.norm(d) * 0.93 * r
            mode2 = b == 0 and m % 5 >= 3                  # blob 0: two rotation modes 40 degrees apart, 3 : 2
            poses.append(_pose(_jitter(rng, Rb2 if mode2 else Rb), t))
            votes.append(int(rng.integers(24, 41)))
    for _ in range(n_clutter):
        poses.append(_pose(rot(rng.normal(size=3), rng.uniform(0.0, 3.1)), rng.uniform(-2.0, 2.0, size=3)))
        votes.append(int(rng.integers(15, 26)))
    poses, votes = np.asarray(poses).reshape(-1, 4, 4), np.asarray(votes, dtype=np.uint32)
    if distinct:
        votes = (1000 + rng.permutation(len(votes))).astype(np.uint32)
    perm = rng.permutation(len(votes))
    return np.ascontiguousarray(poses[perm]), np.ascontiguousarray(votes[perm])


def _split_rotation(seed):
    rng = np.random.default_rng(seed)
    Ra = rot([1.0, 2.0, -0.5], 0.9)
    Rb = Ra @ rot([0.0, 1.0, 1.0], 40.0 * DEG)
    poses, votes = [], []
    for m in range(60):
        poses.append(_pose(_jitter(rng, Ra if m < 34 else Rb), np.array([0.2, 0.1, -0.3]) + _ball(rng, 0.3 * R_DIST)))
        votes.append(int(rng.integers(20, 31)))
    perm = rng.permutation(60)
    return np.asarray(poses)[perm], np.asarray(votes, dtype=np.uint32)[perm]


def _bridge(seed):
    """two clusters, each a tight blob of 12 with an arm pose 0.7 r towards the other; between the arms a pose that neighbours
    both arms and nothing else: no core, with core neighbours in two clusters.  The cluster on the right has the higher votes, so
    its cores come first."""
    rng = np.random.default_rng(seed)
    r = R_DIST
    R0 = rot([0.2, 0.4, 1.0], 0.5)
    poses, votes = [], []
    for side, x0, arm, lo in ((0, 0.0, 0.7 * r, 20), (1, 2.9 * r, 2.2 * r, 30)):
        for _ in range(12):
            poses.append(_pose(_jitter(rng, R0, 2.0), np.array([x0, 0.0, 0.0]) + _ball(rng, 0.02 * r)))
            votes.append(lo + int(rng.integers(0, 8)))
        poses.append(_pose(_jitter(rng, R0, 2.0), np.array([arm, 0.0, 0.0]) + _ball(rng, 0.01 * r)))
        votes.append(lo + 8)
    poses.append(_pose(_jitter(rng, R0, 2.0), np.array([1.45 * r, 0.0, 0.0])))
    votes.append(25)
    perm = rng.permutation(len(votes))
    return np.asarray(poses)[perm], np.asarray(votes, dtype=np.uint32)[perm]


def _chain(seed):
    rng = np.random.default_rng(seed)
    R0 = rot([1.0, 0.0, 0.3], 1.1)
    d = np.array([0.6, 0.64, 0.48])
    d = d / np.linalg.norm(d)
    poses = np.asarray([_pose(R0, np.array([-0.5, 0.2, 0.1]) + d * (0.6 * R_DIST * m) + _ball(rng, 0.01 * R_DIST)) for m in range(300)])
    return poses, (1000 + rng.permutation(300)).astype(np.uint32)      # (distinct: the sorted order scrambles the line)


def _ties(seed):
    rng = np.random.default_rng(seed)
    poses = []
    for b in range(2):
        Rb = rot([0.1 + b, 1.0, 0.2], 0.7 + b)
        for _ in range(14):
            poses.append(_pose(_jitter(rng, Rb), np.array([0.5 * b, 0.1, 0.0]) + _ball(rng, 0.3 * R_DIST)))
    return np.asarray(poses)[rng.permutation(28)], np.full(28, 5, np.uint32)


def _threshold(seed):
    rng = np.random.default_rng(seed)
    R0 = rot([0.5, 0.5, 1.0], 0.3)
    votes = [41, 35, 33, 30, 28, 27, 26, 25, 24, 23, 22, 21, 20, 20, 20, 19, 19, 19, 19]   # size_t(41 * 0.5) = 20: the 19s are cut
    poses = [_pose(_jitter(rng, R0), np.array([0.1, 0.2, 0.3]) + _ball(rng, 0.3 * R_DIST)) for _ in votes]
    perm = rng.permutation(len(votes))
    return np.asarray(poses)[perm], np.asarray(votes, dtype=np.uint32)[perm]


def _identical(seed):
    rng = np.random.default_rng(seed)
    A = _pose(rot([1.0, 1.0, 0.2], 0.8), [0.3, 0.1, -0.2])
    B = _pose(rot([0.0, 1.0, 0.7], 2.1), [-0.4, 0.0, 0.5])
    poses = np.asarray([A] * 9 + [B] * 8)
    return poses, rng.integers(10, 20, size=17).astype(np.uint32)


def _opposite(seed):
    rng = np.random.default_rng(seed)
    Ra = rot([0.3, 1.0, -0.4], 0.6)
    Rb = Ra @ rot([1.0, 0.0, 0.0], np.pi)
    poses, votes = [], []
    for m in range(22):
        poses.append(_pose(_jitter(rng, Ra if m < 12 else Rb, 2.0), np.array([0.0, 0.3, 0.1]) + _ball(rng, 0.3 * R_DIST)))
        votes.append(int(rng.integers(20, 30)))
    return np.asarray(poses), np.asarray(votes, dtype=np.uint32)


def _sparse(seed):
    rng = np.random.default_rng(seed)
    poses = []
    for m in range(20):                                   # twenty pairs, 3 r apart: no pose has three neighbours
        c = np.array([m % 5, (m // 5) % 4, 0.0]) * 3.0 * R_DIST
        for _ in range(2):
            poses.append(_pose(rot(rng.normal(size=3), rng.uniform(0, 3)), c + _ball(rng, 0.25 * R_DIST)))
    return np.asarray(poses), rng.integers(10, 20, size=40).astype(np.uint32)


FAMILIES = (tuple("blobs_%d" % p for p in BLOB_SIZES) + ("distinct_257", "distinct_600", "split_rotation", "bridge", "chain", "ties",
                                                        "threshold", "identical", "opposite", "sparse", "single"))
DISTINCT_VOTES = ("distinct_257", "distinct_600", "chain")      # the families a shuffled input must give equal results on


@functools.lru_cache(maxsize=None)
def family(name):
    """-> (poses (P, 4, 4), votes (P,) uint32); dist_threshold = R_DIST and angle_threshold = ANGLE for all"""
    if name.startswith("blobs_"):
        p = int(name[6:])
        out = _blobs(p, 100 + p)
    elif name.startswith("distinct_"):
        p = int(name[9:])
        out = _blobs(p, 300 + p, distinct=True)
    elif name == "single":
        out = (np.asarray([_pose(rot([0, 0, 1.0], 0.4), [0.1, 0.2, 0.3])]), np.asarray([7], dtype=np.uint32))
    else:
        out = {"split_rotation": _split_rotation, "bridge": _bridge, "chain": _chain, "ties": _ties, "threshold": _threshold,
               "identical": _identical, "opposite": _opposite, "sparse": _sparse}[name](7)
    poses, votes = np.ascontiguousarray(out[0], dtype=np.float64), np.ascontiguousarray(out[1], dtype=np.uint32)
    poses.setflags(write=False)
    votes.setflags(write=False)
    return poses, votes


@functools.lru_cache(maxsize=None)
def judged(name):
    return judge(*family(name))


# ---- the end-to-end case: ppf_ref_util's 1 200-point box model posed into clutter
@functools.lru_cache(maxsize=None)
def estimate_case():
    """-> dict(points, normals, diameter, r_min, scene_points, scene_normals, reference, T): the box posed by T, 1 500 clutter
    points, every fourth of the copy's points a reference point"""
    import ppf_ref_util as U

    pts, nrm, diameter = U.family("box", 1200, 13)
    T = U.pose(3)
    sp, sn, where = U.scene_of(pts, nrm, T, 1500, 3)
    return dict(points=pts, normals=nrm, diameter=diameter, r_min=0.45 * diameter, scene_points=sp, scene_normals=sn,
                reference=np.sort(where[::4]).astype(np.int64), T=T)


@functools.lru_cache(maxsize=None)
def estimate_case_two():
    """two copies of the box, posed by Ta and Tb two diameters apart, in 1 500 clutter points: two translation clusters, two ICP
    calls, two results -> estimate_case's dict with T = (Ta, Tb)"""
    import ppf_ref_util as U

    pts, nrm, diameter = U.family("box", 1200, 13)
    Ta, Tb = U.pose(3), U.pose(8)
    Tb[:3, 3] += np.array([2.0 * diameter, 0.0, 0.0])
    rng = np.random.default_rng(2024)
    sp = np.vstack([pts @ T[:3, :3].T + T[:3, 3] for T in (Ta, Tb)])
    sn = np.vstack([nrm @ T[:3, :3].T for T in (Ta, Tb)])
    cp = rng.uniform(sp.min(axis=0) - 0.3, sp.max(axis=0) + 0.3, size=(1500, 3))
    cn = rng.normal(size=(1500, 3))
    cn /= np.linalg.norm(cn, axis=1, keepdims=True)
    # the second copy is voted at fewer reference points: its cluster has the fewer votes
    ref = np.concatenate([np.arange(0, 1200, 4), 1200 + np.arange(0, 1200, 6)]).astype(np.int64)
    return dict(points=pts, normals=nrm, diameter=diameter, r_min=0.45 * diameter, scene_points=np.ascontiguousarray(np.vstack([sp, cp])),
                scene_normals=np.ascontiguousarray(np.vstack([sn, cn])), reference=ref, T=(Ta, Tb))
