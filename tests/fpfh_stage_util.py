"""The references of the FPFH stage tests (tests/test_fpfh.py, tests/test_gpu_fpfh_stages.py) in plain numpy on top of the C
restatement (fpfh_ref_util.Ref), and the clouds both files run.

The call is cut where m3d_bench_fpfh_stages cuts it: the lists (Ref.neighbours), the SPFH rows as INTEGER pair counts + one
increment per row (ref_counts), which points may be near ties of the acos comparison (tie_bands), and the gather of
fpfh_fpfh_k as a fixed sequence of IEEE operations on given lists, counts and increments (assemble).

Every numpy expression below is one rounded operation per element (numpy does not contract), and `dot` is the contract's
(a0 b0 + a1 b1) + a2 b2."""
import functools
import math

import numpy as np

import fpfh_ref_util as U

EDGE = 1e-9          # "near a bin edge": the project's figure (ppf_ref_util, DESIGN.md "PPF voting")
EPS = 2.220446049250313e-16
INNER, LIB, OUTER = 32.0, 64.0, 128.0       # tie bands in eps; the library's is 64 (kFpfhTieBand)
_CHUNK = 400_000


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def pair_table(idx, cnt):
    """the pairs SPFH counts: entries 1 .. m-1 of every list (entry 0 is skipped whoever it is) -> (owner, k, neighbour)"""
    idx = np.asarray(idx)
    kk = np.arange(idx.shape[1])[None, :]
    own, k = np.nonzero((kk >= 1) & (kk < np.asarray(cnt).astype(np.int64)[:, None]))
    return own, k, idx[own, k].astype(np.int64)


def _pairs12(pts, nrm, own, j):
    return np.concatenate([pts[own], nrm[own], pts[j], nrm[j]], 1)


def ref_pairs(ref, pts, nrm, idx, cnt):
    """-> (owner, k, neighbour, bins (P, 3), features (P, 3)) of every counted pair, by the restatement"""
    own, k, j = pair_table(idx, cnt)
    bins = np.zeros((len(own), 3), np.int32)
    feat = np.zeros((len(own), 3))
    for a in range(0, len(own), _CHUNK):
        s = slice(a, a + _CHUNK)
        bins[s], feat[s] = ref.pair_bins(_pairs12(pts, nrm, own[s], j[s]))
    return own, k, j, bins, feat


def counts_of(n, own, bins):
    flat = (own[:, None] * 33 + bins).ravel()
    return np.bincount(flat, minlength=33 * n).reshape(n, 33).astype(np.int64)


def ref_counts(ref, pts, nrm, search, radius, k, lists=None):
    """the SPFH rows as integers: (counts int64 (n, 33), m int64 (n,)); lists = Ref.neighbours(...) if already at hand"""
    idx, _, m = lists if lists is not None else ref.neighbours(pts, search, radius, k)
    own, _, _, bins, _ = ref_pairs(ref, pts, nrm, idx, m)
    return counts_of(len(pts), own, bins), m.astype(np.int64)


def incr_of(m):
    m = np.asarray(m).astype(np.int64)
    return np.where(m > 1, 100.0 / np.maximum(m - 1, 1).astype(np.float64), 0.0)


def bin_coordinates(features):
    f = np.asarray(features, np.float64)
    return np.stack([11.0 * (f[:, 0] + np.pi) / (2.0 * np.pi), 11.0 * (f[:, 1] + 1.0) / 2.0, 11.0 * (f[:, 2] + 1.0) / 2.0], 1)


def undecided(features):
    """per pair: one of the three bin coordinates lies within EDGE of an integer edge 1 .. 10"""
    x = bin_coordinates(features)
    r = np.rint(x)
    return ((np.abs(x - r) <= EDGE) & (r >= 1) & (r <= 10)).any(1)


def tie_bands(pts, nrm, lists):
    """lists = (idx, cnt).  Per point: has a pair with x1 != x2, d != 0 and |acos x1 - acos x2| <= c eps max(acos x1, acos x2),
    -> (inner, library, outer) boolean arrays for c = 32, 64, 128"""
    idx, cnt = lists
    n = len(pts)
    own, _, j = pair_table(idx, cnt)
    out = [np.zeros(n, bool) for _ in range(3)]
    with np.errstate(invalid="ignore", divide="ignore"):
        for a in range(0, len(own), _CHUNK):
            o, jj = own[a:a + _CHUNK], j[a:a + _CHUNK]
            dp = pts[jj] - pts[o]
            d = np.sqrt(_dot(dp, dp))
            x1 = np.abs(_dot(nrm[o], dp) / d)
            x2 = np.abs(_dot(nrm[jj], dp) / d)
            # |acos x1 - acos x2| >= |x1 - x2|, so a pair in the widest band (128 eps x pi / 2 < 5e-14) has |x1 - x2| < 1e-12;
            # the few that pass go through the C library's acos, the contract's, one at a time
            near = np.nonzero((d != 0) & (x1 != x2) & (np.abs(x1 - x2) <= 1e-12))[0]
            for t in near:
                if x1[t] > 1.0 or x2[t] > 1.0:                       # NaN on the device: every comparison false
                    continue
                y1, y2 = math.acos(x1[t]), math.acos(x2[t])
                for band, c in zip(out, (INNER, LIB, OUTER)):
                    if abs(y1 - y2) <= (c * EPS) * max(y1, y2):
                        band[o[t]] = True
    return tuple(out)


def assemble(list_idx, list_d2, cnt, spfh_count, spfh_incr):
    """fpfh_fpfh_k on given lists, counts and increments, operation for operation -> (n, 33)"""
    idx = np.asarray(list_idx).astype(np.int64)
    d2 = np.asarray(list_d2, np.float64)
    m = np.asarray(cnt).astype(np.int64)
    n = len(m)
    spfh = np.asarray(spfh_count).astype(np.float64) * np.asarray(spfh_incr, np.float64)[:, None]      # count x incr
    acc = np.zeros((n, 33))
    for k in range(1, int(m.max()) if n else 0):
        use = np.nonzero((k < m) & (d2[:, k] != 0.0))[0]
        if len(use):
            acc[use] = acc[use] + spfh[idx[use, k]] / d2[use, k][:, None]
    out = np.zeros((n, 33))
    for g in range(3):
        s = np.zeros(n)
        for b in range(11):                                         # ascending bin order
            s = s + acc[:, 11 * g + b]
        with np.errstate(divide="ignore"):
            scale = np.where(s != 0.0, 100.0 / s, 0.0)
        out[:, 11 * g:11 * g + 11] = acc[:, 11 * g:11 * g + 11] * scale[:, None] + spfh[:, 11 * g:11 * g + 11]
    out[m <= 1] = 0.0
    return out


# ---- clouds ---------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _case(name, pts, nrm, search, radius, k, **extra):
    return dict(name=name, pts=np.ascontiguousarray(pts, np.float64), nrm=np.ascontiguousarray(nrm, np.float64), search=search,
                radius=float(radius), k=int(k), **extra)


NONFINITE_ROWS = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan],
                           [np.inf, -np.inf, 0.0], [0.0, np.nan, np.inf], [-np.inf, 1.0, 2.0]])


def with_nonfinite(pts, nrm):
    """7 non-finite rows scattered through the cloud (the first and the last row among them) -> (pts, nrm, kept positions)"""
    total = len(pts) + 7
    bad = np.unique(np.rint(np.linspace(0, total - 1, 7)).astype(np.int64))
    assert len(bad) == 7
    keep = np.setdiff1d(np.arange(total), bad)
    p = np.zeros((total, 3))
    q = np.tile([0.0, 0.0, 1.0], (total, 1))
    p[bad] = NONFINITE_ROWS
    p[keep] = pts
    q[keep] = nrm
    return p, q, keep


GROUP_SIZES = (1, 2, 3, 4, 64, 65, 66, 128)
M_VALUES = (0, 1, 2, 3, 4, 64, 65, 66, 128)
N_FINITE = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257)
MAX_NN = (1, 2, 16, 17, 32, 33, 64, 65, 127, 128)


def grouped_cloud(seed=41):
    """balls of diameter 0.4, three units apart, holding 1, 2, 3, 4, 64, 65, 66 and 128 points, in shuffled order: under
    Hybrid(0.5, 128) every point's m is the size of its ball"""
    rng = np.random.default_rng(seed)
    pts, size = [], []
    for g, s in enumerate(GROUP_SIZES):
        pts.append(np.array([3.0 * g, 0.0, 0.0]) + 0.2 * _unit(rng, s) * rng.uniform(0, 1, (s, 1)) ** (1 / 3))
        size += [s] * s
    pts = np.concatenate(pts)
    perm = rng.permutation(len(pts))
    return pts[perm], _unit(rng, len(pts)), np.array(size)[perm]


@functools.lru_cache(maxsize=None)
def seam_cases():
    """name -> case; the smallest shapes at which each kernel of the chain can still go wrong"""
    cases = []
    rng = np.random.default_rng(77)
    # own neighbour count m: KNN(128) on clouds of exactly m finite points, Hybrid on the grouped cloud, m = 0 by radius 0
    for m in M_VALUES[1:]:
        p, q = U.three_surface_cloud(max(m, 3), seed=100 + m)
        cases.append(_case(f"m{m}_knn", p[:m], q[:m], U.KNN, 0.0, 128, m_all=m))
    gp, gq, gsize = grouped_cloud()
    cases.append(_case("m_grouped_hybrid", gp, gq, U.HYBRID, 0.5, 128, m_each=gsize))
    cases.append(_case("m0_radius0", gp[:70], gq[:70], U.HYBRID, 0.0, 30, m_all=0))
    # query counts, each again with 7 non-finite rows scattered through it
    for n in N_FINITE:
        p, q = U.three_surface_cloud(max(n, 3), seed=200 + n)
        p, q = p[:n], q[:n]
        cases.append(_case(f"n{n}", p, q, U.HYBRID, 2.0, 17))
        p2, q2, keep = with_nonfinite(p, q)
        cases.append(_case(f"n{n}_nonfinite", p2, q2, U.HYBRID, 2.0, 17, base=f"n{n}", keep=keep))
    # list lengths: the KCAP templates and grid classes; and max_nn above the number of finite points
    lp, lq = U.three_surface_cloud(300, seed=31)
    for k in MAX_NN:
        cases.append(_case(f"max_nn{k}", lp, lq, U.KNN, 0.0, k))
    cases.append(_case("max_nn_above_n_knn", lp[:40], lq[:40], U.KNN, 0.0, 64, m_all=40))
    cases.append(_case("max_nn_above_n_hybrid", lp[:40], lq[:40], U.HYBRID, 100.0, 128, m_all=40))
    # the Hybrid cut at equality: r2 = 4.0 exactly, then the next double
    lat = U.lattice(6)
    ln = _unit(np.random.default_rng(9), len(lat))
    cases.append(_case("lattice_r2_out", lat, ln, U.HYBRID, 2.0, 40, m_max=27))
    cases.append(_case("lattice_r2_in", lat, ln, U.HYBRID, np.nextafter(2.0, 3.0), 40, m_max=33))
    # the u8 count's ceiling: 127 pairs in each of three bins
    flat = np.concatenate([np.random.default_rng(3).uniform(-1, 1, size=(600, 2)), np.zeros((600, 1))], 1)
    cases.append(_case("flat_knn128", flat, np.tile([0.0, 0.0, 1.0], (600, 1)), U.KNN, 0.0, 128, flat=True))
    # duplicates: three and five copies inside an ordinary cloud (lowest and highest index among them), one point 70 times
    dp, dq = U.three_surface_cloud(500, seed=51)
    dp[250] = dp[499] = dp[0]
    dp[100] = dp[200] = dp[300] = dp[498] = dp[1]
    cases.append(_case("duplicates", dp, dq, U.HYBRID, 0.3, 50, copies=((0, 250, 499), (1, 100, 200, 300, 498))))
    cases.append(_case("one_point_70", np.tile([0.3, -0.7, 1.1], (70, 1)), _unit(rng, 70), U.KNN, 0.0, 100, m_all=70))
    # degenerate normals
    cases.append(_case("collinear3", np.array([[0.1, 0.2, 0.3], [0.4, 0.8, 1.2], [0.2, 0.4, 0.6]]), _unit(rng, 3), U.KNN, 0.0, 3,
                       m_all=3))
    far = np.concatenate([rng.uniform(-1, 1, size=(400, 2)), np.zeros((400, 1))], 1) + np.array([1000.0, -2000.0, 3000.0])
    cases.append(_case("far_plane", far, _unit(rng, 400), U.KNN, 0.0, 30))
    return {c["name"]: c for c in cases}


@functools.lru_cache(maxsize=None)
def big_cases():
    """the three-surface cloud under the parameter sets of test_gpu_fpfh.py::test_fpfh_matches_restatement, given normals"""
    p, q = U.three_surface_cloud(20000)
    return {f"big_{s}_{r}_{k}": _case(f"big_{s}_{r}_{k}", p, q, s, r, k)
            for s, r, k in ((U.HYBRID, 0.1, 100), (U.HYBRID, 0.05, 30), (U.KNN, 0.0, 30), (U.KNN, 0.0, 128))}


_TIE_CASES = {}


def tie_cases(ref):
    """clouds with ESTIMATED normals (the restatement's, oriented to the origin): neighbouring normals agree to an ulp and the
    acos comparison has near ties.  tie6000: the cloud of test_end_to_end_registration under preprocess_fragment's searches;
    tie6000_moved: that test's second cloud, the first one moved and permuted -- the cloud on which the device's acos and the
    host's were first seen to order a pair differently ("FPFH"); tie1500: KNN(128), lists fpfh_tie_gather_k strides
    twice."""
    if not _TIE_CASES:
        from misc3d_amd import synth
        p, _ = U.three_surface_cloud(6000, seed=21)
        q = ref.normals(p, U.HYBRID, 0.08, 30, orient_to=(0, 0, 0))
        _TIE_CASES["tie6000"] = _case("tie6000", p, q, U.HYBRID, 0.2, 100, estimated=True)
        T = synth.rigid_transform(25.0, (1, 2, 3), (0.2, -0.1, 0.3))
        p = np.ascontiguousarray((p @ T[:3, :3].T + T[:3, 3])[np.random.default_rng(2).permutation(len(p))])
        q = ref.normals(p, U.HYBRID, 0.08, 30, orient_to=(0, 0, 0))
        _TIE_CASES["tie6000_moved"] = _case("tie6000_moved", p, q, U.HYBRID, 0.2, 100, estimated=True)
        p, _ = U.three_surface_cloud(1500, seed=22)
        q = ref.normals(p, U.HYBRID, 0.2, 30, orient_to=(0, 0, 0))
        _TIE_CASES["tie1500"] = _case("tie1500", p, q, U.KNN, 0.0, 128, estimated=True)
    return _TIE_CASES


# Points with a pair inside the 32 / 64 / 128 eps bands, as tests/test_fpfh.py::test_stage_inputs_have_no_undecided_pair
# computes them (filled in from its output; a cloud with given normals has none)
TIE_COUNTS = {"tie6000": (80, 114, 155), "tie6000_moved": (40, 71, 125), "tie1500": (35, 45, 63)}

_REFS = {}


def reference(ref, case):
    """everything the stage tests hold a case to, computed once per process: lists, pair table, counts, bands, whole call"""
    name = case["name"]
    if name not in _REFS:
        pts, nrm = case["pts"], case["nrm"]
        idx, d2, m = ref.neighbours(pts, case["search"], case["radius"], case["k"])
        own, k, j, bins, feat = ref_pairs(ref, pts, nrm, idx, m)
        _REFS[name] = dict(idx=idx, d2=d2, m=m.astype(np.int64), own=own, k=k, j=j, bins=bins, feat=feat,
                           counts=counts_of(len(pts), own, bins), undecided=undecided(feat), bands=tie_bands(pts, nrm, (idx, m)))
    return _REFS[name]
