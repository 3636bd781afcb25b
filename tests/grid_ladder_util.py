"""Scenes that put every radius-grid search on a chosen rung of the cell-table ladder (radius_grid_geom, m3d_grid_geom.hpp), and a
python restatement of that ladder.

The ladder: cell edge h = 1.001 edge / K with K = K0; while the dense table exceeds 2^27 cells K is halved and h recomputed, and
once K == 1 the cell is doubled.  Its invariant -- K h >= 1.001 edge, so the (2K + 1)^3 block around a query's cell holds
everything within `edge` -- is what every consumer's kernels take on trust.  Which rung a scene lands on depends only on
extent / edge and K0, so every scene here is `islands` of a few hundred points spaced far apart: a few thousand points span a box
of 10 to 1e10 radii.  All scenes have extent EXTENT whatever the ratio (the radius shrinks instead): the tolerances of the
consumers' existing tests are absolute.

Island content:
  volumetric   uniform in cubes of edge 12 r (1 to 2 points per radius ball), queries = every second point moved by N(0, 0.45 r)
               per coordinate: most have a neighbour within r, many of them between 2/3 r and r away and diagonally placed
  surface      gently curved patches of edge 12 r with analytic normals, 10 to 40 points per radius ball (below the 128-neighbour
               cap of boundary detection's Radius search)
Variants: `flat` (all z equal: the table is seven cells thick and the cap is reached near extent / r = 6000 instead of 500),
`shift` (one island moved by a non-integer number of cells, so that the islands straddle the cell faces differently), `room`
(six patches on the faces of the box: the sparse room of DESIGN.md's benchmark S4, extent / r = 2000, at small size).
Every scene carries a handful of exact duplicates (appended: the higher index of each tie) and, on request, one non-finite row."""
import functools
import math

import numpy as np

EXTENT = 2.0
ISLAND = 12.0                      # island edge in radii
CAP = 1 << 27


# ---------------------------------------------------------------------------------------------- the ladder, restated
def ladder_geom(lo, hi, edge, k0):
    """radius_grid_geom -> (K, h, (nx, ny, nz)); finite boxes and edges only"""
    K = int(k0)
    h = edge * 1.001 / K
    while True:
        fits, cells, dims = True, 1, []
        for k in range(3):
            ext = (float(hi[k]) - float(lo[k])) / h
            if not ext < 1e9:
                fits = False
                break
            dims.append(int(ext) + 1 + 2 * (2 * K + 1))
            cells *= dims[-1]
            if cells > CAP:
                fits = False
        if fits:
            return K, h, tuple(dims)
        if K > 1:
            K //= 2
            h = edge * 1.001 / K
        else:
            h *= 2.0


def reg_grid_k0(k_cfg, n_dst):
    """reg_grid_k0 (m3d_grid_geom.hpp): std::lround rounds halves away from zero"""
    return max(1, min(int(k_cfg), int(math.floor(k_cfg * (n_dst / 200000.0) ** (1.0 / 3.0) + 0.5))))


def bbox(pts):
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    return p.min(axis=0), p.max(axis=0)


def rung(pts, edge, k0, hook=ladder_geom):
    """-> (K, doublings of the cell, h): the rung the cloud's grid lands on"""
    lo, hi = bbox(pts)
    K, h, dims = hook(lo, hi, edge, k0)
    assert dims[0] * dims[1] * dims[2] <= CAP
    return K, int(round(math.log2(h * K / (1.001 * edge)))), h


# ---------------------------------------------------------------------------------------------- island layouts
CORNERS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1))
FLAT_CORNERS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0.5, 0.5, 0))
ROOM_FACES = ((0.5, 0.5, 0), (0.5, 0.5, 1), (0.5, 0, 0.5), (0.5, 1, 0.5), (0, 0.5, 0.5), (1, 0.5, 0.5))
SIZES = (700, 650, 600, 550, 500)


def layout(ratio, variant="cubic", island=ISLAND):
    """-> (r, s, origins): the radius, the islands' edge s and the low corner of each island's cube.  The islands' cubes span
    EXTENT = ratio r on every axis a variant uses."""
    r = EXTENT / ratio
    s = min(island, 0.3 * ratio) * r
    span = EXTENT - s
    corners = {"cubic": CORNERS, "shift": CORNERS, "flat": FLAT_CORNERS, "room": ROOM_FACES}[variant]
    origins = np.array(corners, np.float64) * span
    if variant == "shift":                          # off the lattice of every rung's cells, inside the box on every axis
        origins[1] += np.array([-0.37, 0.61, 0.13]) * 1.001 * r * 2.0 ** max(0, math.ceil(math.log2(max(ratio / 500.0, 1.0))))
    return r, s, origins


def _finish(rng, pts, extra, n_dup, nonfinite):
    """appends n_dup exact copies of even-index rows (with their rows of `extra`) and, on request, one non-finite row"""
    n = len(pts)
    src = rng.choice(np.arange(0, n, 2), n_dup, replace=False)
    pts = np.vstack([pts, pts[src]])
    extra = None if extra is None else np.vstack([extra, extra[src]])
    if nonfinite:
        pts = np.vstack([pts, [[np.nan, 0.5, np.inf]]])
        extra = None if extra is None else np.vstack([extra, [[0.0, 0.0, 1.0]]])
    c = np.ascontiguousarray
    return c(pts), (None if extra is None else c(extra)), src


@functools.lru_cache(maxsize=None)
def volumetric(ratio, variant="cubic", sizes=SIZES, island=ISLAND, seed=1, n_dup=8, nonfinite=False):
    """-> dict(pts, r, dup_of (the rows the last n_dup finite rows copy), island (per row))"""
    rng = np.random.default_rng(seed)
    r, s, origins = layout(ratio, variant, island)
    pts, isl = [], []
    for k, (o, m) in enumerate(zip(origins, sizes)):
        p = o + rng.uniform(0.0, s, (m, 3))
        if variant == "flat":
            p[:, 2] = 0.25
        pts.append(p)
        isl.append(np.full(m, k))
    pts, _, dup_of = _finish(rng, np.vstack(pts), None, n_dup, nonfinite)
    return dict(pts=pts, r=r, dup_of=dup_of, island=np.concatenate(isl), variant=variant, ratio=ratio)


def queries(scene, seed=2):
    """every second finite row of the scene moved by N(0, 0.45 r) per coordinate"""
    rng = np.random.default_rng(seed)
    p = scene["pts"][: len(scene["island"])][::2]
    return np.ascontiguousarray(p + rng.normal(0.0, 0.45 * scene["r"], p.shape))


@functools.lru_cache(maxsize=None)
def surface(ratio, variant="cubic", sizes=SIZES, seed=3, n_dup=6, nonfinite=True):
    """patches z = a x^2 + b x y (local, in units of the patch edge) turned onto a face per island, with analytic unit normals
    -> dict(pts, normals, r, island)"""
    rng = np.random.default_rng(seed)
    r, s, origins = layout(ratio, variant)
    pts, nrm, isl = [], [], []
    for k, (o, m) in enumerate(zip(origins, sizes)):
        uv = rng.uniform(0.0, 1.0, (m, 2))
        a, b = (0.0, 0.0) if variant == "flat" else rng.uniform(-0.08, 0.08, 2)
        w = a * (uv[:, 0] - 0.5) ** 2 + b * (uv[:, 0] - 0.5) * (uv[:, 1] - 0.5) + (0.0 if variant == "flat" else 0.5)
        g = np.stack([-(2 * a * (uv[:, 0] - 0.5) + b * (uv[:, 1] - 0.5)), -b * (uv[:, 0] - 0.5), np.ones(m)], axis=1)
        g /= np.linalg.norm(g, axis=1, keepdims=True)
        local = np.stack([uv[:, 0], uv[:, 1], w], axis=1)
        axes = [0, 1, 2] if variant == "flat" else np.roll([0, 1, 2], k % 3).tolist()      # which world axis the patch faces
        p = np.empty((m, 3))
        q = np.empty((m, 3))
        p[:, axes] = local * s
        q[:, axes] = g
        pts.append(o + p)
        nrm.append(q)
        isl.append(np.full(m, k))
    if variant == "flat":
        for p in pts:
            p[:, 2] = 0.25
    pts, nrm, dup_of = _finish(rng, np.vstack(pts), np.vstack(nrm), n_dup, nonfinite)
    return dict(pts=pts, normals=nrm, r=r, island=np.concatenate(isl), dup_of=dup_of, variant=variant, ratio=ratio)


# ---------------------------------------------------------------------------------------------- registration problems
def rigid(angle_deg=25.0, axis=(0.2, -0.3, 1.0), t=(0.05, -0.02, 0.01)):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    th = np.deg2rad(angle_deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


def apply(T, p):
    return np.ascontiguousarray(p @ T[:3, :3].T + T[:3, 3])


@functools.lru_cache(maxsize=None)
def reg_problem(ratio, variant="cubic", n_target=3000, island=ISLAND, n_noisy=700, n_anchor=300, n_rim=300, n_corr=300, max_iter=400,
                seed=5):
    """A RANSAC registration whose validation runs on the scene's grid: the target is the volumetric scene, the source (moved by
    the inverse of a rigid pose) holds `n_anchor` target points with little noise (0.03 r: the correspondences come from these, so
    that the winning pose is good to a fraction of r) and `n_noisy` with N(0, 0.45 r): what the validation counts.  Half of the
    correspondences are true.  -> dict(src, dst, cs, cd, thr, kw)"""
    rng = np.random.default_rng(seed)
    sizes = tuple(int(round(n_target * m / sum(SIZES))) for m in SIZES)
    sc = volumetric(ratio, variant, sizes, island, seed)
    dst, r = sc["pts"], sc["r"]
    n = len(sc["island"])
    a_idx = rng.choice(n, n_anchor, replace=False)
    q_idx = rng.choice(n, min(n_noisy, n), replace=False)
    # ... and `n_rim` just outside the islands' faces, edges and corners, 0.6 r to 0.98 r out: however dense the target, their
    # nearest target point is about that far away, along an axis or a diagonal of the grid
    _, s, origins = layout(ratio, variant, island)
    d = rng.integers(-1, 2, (n_rim, 3)).astype(np.float64)
    d[(d == 0).all(axis=1)] = [1.0, 1.0, 1.0]
    base = origins[rng.integers(0, len(sizes), n_rim)] + s * np.where(d > 0, 1.0, np.where(d < 0, 0.0, rng.uniform(0, 1, (n_rim, 3))))
    if variant == "flat":
        base[:, 2] = 0.25
    rim = base + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.6, 0.98, (n_rim, 1)) * r
    world = np.vstack([dst[a_idx] + rng.normal(0, 0.03 * r, (n_anchor, 3)), dst[q_idx] + rng.normal(0, 0.45 * r, (len(q_idx), 3)), rim])
    Tm = rigid()
    src = apply(np.linalg.inv(Tm), world)
    cs = rng.integers(0, n_anchor, n_corr)
    cd = np.where(rng.random(n_corr) < 0.5, a_idx[cs], rng.integers(0, n, n_corr))
    return dict(src=src, dst=dst, cs=cs, cd=cd, thr=r, T=Tm, r=r, n_anchor=n_anchor,
                kw=dict(max_iter=max_iter, edge_length_threshold=0.9, confidence=1.0, seed=7))


def nearest_d2(moved, dst):
    """exact-enough nearest distances for the non-vacuity conditions (a k-d tree over the finite target rows)"""
    from scipy.spatial import cKDTree
    fin = np.isfinite(dst).all(axis=1)
    d, _ = cKDTree(dst[fin]).query(moved)
    return d


# ---------------------------------------------------------------------------------------------- ICP problems
@functools.lru_cache(maxsize=None)
def icp_problem(ratio, variant="cubic", seed=9):
    """-> dict(src, dst, dst_normals, max_dist, init, T, max_iteration, dup_of): the queries of the volumetric scene moved back by a
    rigid pose, the initial pose off by 0.15 r; the target carries exact duplicates at its end and one non-finite row"""
    sc = volumetric(ratio, variant, seed=seed, nonfinite=True)
    dst, r = sc["pts"], sc["r"]
    isl, n = sc["island"], len(sc["island"])
    nrm = np.tile([0.0, 0.0, 1.0], (len(dst), 1))
    for k in range(int(isl.max()) + 1):                      # radial about each island's centre: a smooth field
        m = np.flatnonzero(isl == k)
        nrm[m] = dst[m] - dst[m].mean(axis=0)
    nrm[n:n + len(sc["dup_of"])] = np.roll(nrm[sc["dup_of"]], 1, axis=1)      # a copy's normal is not its original's
    nrm[:, 2] += 0.3 * np.linalg.norm(nrm, axis=1)           # (the flat scene's field leaves its plane too)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    T = rigid(40.0, (1, 1, 1), (0.3, -0.1, 0.2))
    q = queries(sc, seed + 2)
    q[sc["dup_of"] // 2] = dst[sc["dup_of"]] + 0.01 * r * np.array([1.0, -1.0, 1.0])   # these meet the exact ties
    src = apply(np.linalg.inv(T), q)
    src[5] = np.nan
    off = rigid(np.rad2deg(0.05 * r / EXTENT), (1.0, -2.0, 0.5), (0.09 * r, -0.08 * r, 0.07 * r))
    return dict(src=src, dst=dst, dst_normals=np.ascontiguousarray(nrm), max_dist=r, init=off @ T, T=T, max_iteration=30,
                dup_of=sc["dup_of"], n_finite=len(sc["island"]), r=r)


@functools.lru_cache(maxsize=None)
def orient_problem(ratio, variant="cubic"):
    """the surface scene without its non-finite row (the call requires finite points), the analytic normals with random signs
    and lengths, the seed in the third island -> dict(points, normals, radius, seed, island (per row))"""
    sc = surface(ratio, variant, ROOM_SIZES if variant == "room" else SIZES, nonfinite=False)
    rng = np.random.default_rng(17)
    n = len(sc["pts"])
    nrm = sc["normals"] * rng.choice([-1.0, 1.0], (n, 1)) * rng.uniform(0.5, 2.0, (n, 1))
    isl = np.concatenate([sc["island"], np.full(n - len(sc["island"]), -1)])
    isl[len(sc["island"]):] = isl[sc["dup_of"]]
    seed = int(np.flatnonzero(isl == 2)[40])
    return dict(points=sc["pts"], normals=np.ascontiguousarray(nrm), radius=sc["r"], seed=seed, island=isl)


# the rungs of the issue's table, (K0, extent / r, variant) -> (K, doublings)
NN_RUNGS = {
    (1, 100, "cubic"): (1, 0), (1, 600, "cubic"): (1, 1), (1, 1200, "cubic"): (1, 2), (1, 3000, "cubic"): (1, 3),
    (1, 1e7, "cubic"): (1, 15), (1, 1e10, "cubic"): (1, 25),
    (1, 3000, "flat"): (1, 0), (1, 8000, "flat"): (1, 1), (1, 1200, "shift"): (1, 2),
    (4, 10, "cubic"): (4, 0), (4, 100, "cubic"): (4, 0), (4, 170, "cubic"): (2, 0), (4, 300, "cubic"): (1, 0),
    (4, 600, "cubic"): (1, 1), (4, 1e7, "cubic"): (1, 15), (4, 3000, "flat"): (1, 0), (4, 600, "shift"): (1, 1),
    (2, 170, "cubic"): (2, 0), (2, 300, "cubic"): (1, 0),
    (3, 100, "cubic"): (3, 0), (3, 170, "cubic"): (1, 0), (3, 300, "cubic"): (1, 0), (3, 600, "cubic"): (1, 1),
    (3, 170, "shift"): (1, 0),
}
K0_1_RUNGS = [k[1:] for k in NN_RUNGS if k[0] == 1]
K0_4_RUNGS = [k[1:] for k in NN_RUNGS if k[0] == 4]
ROOM = (2000, "room")              # DESIGN.md's S4 (a 40 m room at r = 0.02: the cell grows to 4 r) at small size
ROOM_RUNG = (1, 2)
ROOM_SIZES = (550,) * 6
SURFACE_RUNGS = K0_1_RUNGS + [ROOM]


def surface_scene(ratio, variant):
    return surface(ratio, variant, ROOM_SIZES if variant == "room" else SIZES)


def surface_rung(ratio, variant):
    return ROOM_RUNG if variant == "room" else NN_RUNGS[(1, ratio, variant)]


# The registration cases: reg_cells_per_radius = k_cfg on a target of n_target points gives K0 = k0 (reg_grid_k0), and the scene
# puts the validation grid on `rung`.  A 3 000-point target turns k_cfg = 4, 8, 12, 16 into K0 = 1, 2, 3, 4; K0 = 3 at the default
# k_cfg = 4 takes 48 800 to 134 000 points, K0 = 8 at k_cfg = 16 takes 20 600 to 29 900 and K0 = 16 no fewer than 181 900.
def _reg_case(k_cfg, k0, ratio, variant, rung_, n_target=3000, **kw):
    name = "kcfg%d-k0_%d-%g-%s-n%d" % (k_cfg, k0, ratio, variant, n_target)
    return dict(id=name, k_cfg=k_cfg, k0=k0, rung=rung_, problem=dict(ratio=ratio, variant=variant, n_target=n_target, **kw))


_SMALL = dict(n_noisy=150, n_anchor=100, n_rim=200, n_corr=100, max_iter=300)
REG_CASES = [_reg_case(4 * k0, k0, ratio, variant, want) for (k0, ratio, variant), want in NN_RUNGS.items()] + [
    _reg_case(4, 3, 170, "cubic", (1, 0), 55000, n_noisy=500, n_anchor=150, n_rim=500, n_corr=150, max_iter=250),
    _reg_case(16, 8, 50, "cubic", (8, 0), 25000, **_SMALL),
    _reg_case(16, 8, 100, "cubic", (4, 0), 25000, **_SMALL),
    _reg_case(16, 16, 25, "cubic", (16, 0), 184000, **_SMALL),
    _reg_case(16, 16, 50, "cubic", (8, 0), 184000, **_SMALL),
]
FORMERLY_BROKEN = [c["id"] for c in REG_CASES if c["k0"] == 3 and c["problem"]["ratio"] in (170, 300)]

_reg_refs = {}


def reg_reference(orc, case):
    """oracle.registration_ransac on the case's problem, once per problem (it does not depend on k_cfg)"""
    key = tuple(sorted(case["problem"].items()))
    if key not in _reg_refs:
        p = reg_problem(**case["problem"])
        kw = p["kw"]
        _reg_refs[key] = orc.registration_ransac(p["src"], p["dst"], p["cs"], p["cd"], thr=p["thr"], max_iter=kw["max_iter"],
                                                 edge_thr=kw["edge_length_threshold"], confidence=kw["confidence"], seed=kw["seed"])
    return _reg_refs[key]
