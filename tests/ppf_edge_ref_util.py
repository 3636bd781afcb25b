"""The cases both EdgePoints test files use: a sample and an edge set dealt from one ppf_ref_util family, the table shapes, the
vote cases and the end-to-end scene (a flat plate with holes in clutter).  The restatement (tests/cpp/ppf_ref.c) and the judge
take them through ppf_ref_util, as they take the SampledPoints cases; tests/test_ppf_edge.py holds the restatement to the judge on
every case, and checks that no case has a pair within EDGE_BAND of a bin edge."""
import functools

import numpy as np

import ppf_ref_util as pu
from ppf_ref_util import params


# ---- the cases
def split_family(name, n, n_e, seed):
    """n + n_e points of a ppf_ref_util family, dealt by a fixed permutation into the sample (n) and the edge set (n_e): both lie on
    the same surface, as a part's sample and its boundary do -> (points, normals, edge points, edge normals, diameter)"""
    pts, nrm, diameter = pu.family(name, n + n_e, seed)
    perm = np.random.default_rng(5000 + seed).permutation(n + n_e)
    a, b = perm[:n], perm[n:]
    return (np.ascontiguousarray(pts[a]), np.ascontiguousarray(nrm[a]), np.ascontiguousarray(pts[b]), np.ascontiguousarray(nrm[b]),
            diameter)


TABLE_SHAPES = ((2, 1), (3, 2), (2, 3), (63, 65), (65, 63), (64, 64), (257, 255), (255, 257))
TABLE_LARGE = (1500, 700)
TABLE_SEEDS = {(1500, 700): 31}       # (seeds whose pairs are all decided: tests/test_ppf_edge.py checks every one)
VOTE_N = pu.VOTE_N                     # 320 sample points
VOTE_NE = {"random": 320, "sphere": 321, "box": 322, "plate": 323, "grid": 324}     # size_t(0.2 n_e) = 64 for each
VOTE_SEEDS = {"random": 41, "sphere": 42, "box": 43, "plate": 44, "grid": 45}
COUNTS = pu.COUNTS
LDS_EDGE_N = pu.LDS_EDGE_N


@functools.lru_cache(maxsize=None)
def table_case(n, n_e):
    """-> dict(points, normals, edge_points, edge_normals, diameter, r_min, params)"""
    pts, nrm, ept, enr, diameter = split_family("random", n, n_e, TABLE_SEEDS.get((n, n_e), 100 + n))
    return dict(points=pts, normals=nrm, edge_points=ept, edge_normals=enr, diameter=diameter, r_min=0.45 * diameter, params=params())


@functools.lru_cache(maxsize=None)
def coincident_case():
    """64 x 64 with the first 16 edge points ON the sample points of the same index (their normals turned, so that only d2 == 0
    can skip them), the next 16 on sample points of OTHER indices: 32 pairs are skipped, every other equal-index pair is kept"""
    c = dict(table_case(64, 64))
    ept, enr = c["edge_points"].copy(), c["edge_normals"].copy()
    R = pu.pose(77)[:3, :3]
    ept[:16] = c["points"][:16]
    enr[:16] = c["normals"][:16] @ R.T
    ept[16:32] = c["points"][40:56]
    c["edge_points"], c["edge_normals"] = ept, enr
    return c


@functools.lru_cache(maxsize=None)
def _vote_model(name, n=VOTE_N, n_e=None):
    n_e = VOTE_NE[name] if n_e is None else n_e
    pts, nrm, ept, enr, diameter = split_family(name, n, n_e, VOTE_SEEDS[name])
    return pts, nrm, ept, enr, diameter


def _scene(pts, nrm, ept, enr, T, clutter, clutter_e, seed, n_ref):
    sp, sn, where = pu.scene_of(pts, nrm, T, clutter, seed)
    ep, en, _ = pu.scene_of(ept, enr, T, clutter_e, seed + 50)
    ref = np.sort(where[:: max(1, len(pts) // n_ref)][:n_ref])
    return sp, sn, ref.astype(np.int64), ep, en


def _case(model, diameter, r_min, p, scene):
    pts, nrm, ept, enr = model
    sp, sn, ref, ep, en = scene
    return dict(points=pts, normals=nrm, edge_points=ept, edge_normals=enr, diameter=diameter, r_min=r_min, params=p,
                scene_points=sp, scene_normals=sn, reference=np.asarray(ref, dtype=np.int64), scene_edge_points=ep,
                scene_edge_normals=en)


VOTE_CASES = (tuple("family_" + f for f in pu.FAMILIES) + ("step_11.25", "step_6", "full_spread", "full_spread_6") +
              tuple("count_%s_%d" % (f, c) for f in pu.FAMILIES for c in COUNTS) + ("coincident_scene", "lds_edge", "lds_edge_plus_1"))


@functools.lru_cache(maxsize=None)
def case(name):
    """the inputs of one vote case of tests/test_gpu_ppf_edge.py"""
    if name.startswith("family_"):
        fam = name[7:]
        pts, nrm, ept, enr, diameter = _vote_model(fam)
        return _case((pts, nrm, ept, enr), diameter, 0.45 * diameter, params(), _scene(pts, nrm, ept, enr, pu.pose(len(fam)), 400, 150, len(fam), 12))
    if name in ("step_11.25", "step_6", "full_spread", "full_spread_6"):
        fam = {"step_11.25": "box", "step_6": "sphere", "full_spread": "random", "full_spread_6": "box"}[name]
        step = {"step_11.25": "11.25", "step_6": "6", "full_spread": "12", "full_spread_6": "6"}[name]
        pts, nrm, ept, enr, diameter = _vote_model(fam)
        return _case((pts, nrm, ept, enr), diameter, 0.45 * diameter,
                     params(angle_step=pu.ANGLE_STEPS[step], faster_mode=not name.startswith("full")),
                     _scene(pts, nrm, ept, enr, pu.pose(len(fam)), 400, 150, len(fam), 6))
    if name.startswith("count_"):
        _, fam, count = name.split("_")
        pts, nrm, ept, enr, diameter = _vote_model(fam)
        r_min = 1.2 * diameter            # every edge point is a neighbour of every sample point
        T = pu.pose(5)
        sp, sn = pts @ T[:3, :3].T + T[:3, 3], nrm @ T[:3, :3].T
        ep, en = ept @ T[:3, :3].T + T[:3, 3], enr @ T[:3, :3].T
        d = np.linalg.norm(ep - sp[0], axis=1)
        order = np.argsort(d, kind="stable")
        inside = order[d[order] < 0.999 * r_min]
        assert len(inside) >= int(count), (len(inside), count)
        keep = np.concatenate([inside[:int(count)], np.nonzero(d > 1.05 * r_min)[0]])
        # (min_dist_thresh as ppf_ref_util's count cases: the plate's and the grid's normals are parallel)
        return _case((pts, nrm, ept, enr), diameter, r_min, params(min_dist_thresh=0.01),
                     (np.ascontiguousarray(sp), np.ascontiguousarray(sn), [0], np.ascontiguousarray(ep[keep]), np.ascontiguousarray(en[keep])))
    if name == "coincident_scene":
        # every reference point is also a scene edge point, its normal turned: scene pairs with d2 == 0 that pass the filter
        c = dict(case("family_sphere"))
        R = pu.pose(77)[:3, :3]
        ref = c["reference"]
        c["scene_edge_points"] = np.vstack([c["scene_edge_points"], c["scene_points"][ref]])
        c["scene_edge_normals"] = np.vstack([c["scene_edge_normals"], c["scene_normals"][ref] @ R.T])
        return c
    if name in ("lds_edge", "lds_edge_plus_1"):
        n = LDS_EDGE_N + (name != "lds_edge")
        pts, nrm, ept, enr, diameter = split_family("box", n, 322, 46)
        return _case((pts, nrm, ept, enr), diameter, 0.45 * diameter, params(angle_step=pu.ANGLE_STEPS["6"]),
                     _scene(pts, nrm, ept, enr, pu.pose(3), 300, 150, 3, 4))
    raise KeyError(name)


# ---- the end-to-end case: a flat plate with holes in clutter
PLATE_SEED = 7


@functools.lru_cache(maxsize=None)
def plate_with_holes(n_side=40, n_rim=140, n_hole=50, seed=PLATE_SEED, n_wall=180, thickness=0.04):
    """a 1.0 x 0.7 plate with three holes, none placed symmetrically: -> (sample points, normals, edge points, edge normals,
    diameter).  The sample is a jittered grid on the face outside the holes, with the face's normal tilted a few degrees as
    ppf_ref_util's plate family tilts it (a normal exactly perpendicular to every in-plane difference puts f0 = f1 = pi / 2 on a bin
    edge of the 12 degree step), and n_wall points on the walls of the rim and of the holes (the plate is `thickness` thick), whose
    normals lie in the plate: without them no point-to-plane residual sees a slide inside the plane.  The edge set is the rim and
    the holes' circles on the face, with the face's normal."""
    rng = np.random.default_rng(seed)
    a, b, plate_normal, tilted = pu._tilt_frame(rng)
    holes = ((-0.27, 0.12, 0.11), (0.18, -0.14, 0.085), (0.31, 0.19, 0.06))
    u = (np.arange(n_side) + 0.5) / n_side - 0.5
    v = (np.arange(int(n_side * 0.7)) + 0.5) / int(n_side * 0.7) * 0.7 - 0.35
    uv = np.stack(np.meshgrid(u, v, indexing="ij"), axis=-1).reshape(-1, 2)
    uv = uv + rng.uniform(-0.3, 0.3, size=uv.shape) / n_side
    keep = np.ones(len(uv), bool)
    for cx, cy, r in holes:
        keep &= (uv[:, 0] - cx) ** 2 + (uv[:, 1] - cy) ** 2 > (r + 0.4 / n_side) ** 2
    uv = uv[keep]
    t = rng.uniform(0, 3.4, size=n_rim)            # the rim, by arc length: 1.0 + 0.7 + 1.0 + 0.7
    rim = np.where((t < 1.0)[:, None], np.stack([t - 0.5, np.full_like(t, -0.35)], 1),
                   np.where((t < 1.7)[:, None], np.stack([np.full_like(t, 0.5), t - 1.0 - 0.35], 1),
                            np.where((t < 2.7)[:, None], np.stack([2.2 - t, np.full_like(t, 0.35)], 1),
                                     np.stack([np.full_like(t, -0.5), 3.05 - t], 1))))
    rings = []
    for cx, cy, r in holes:
        th = rng.uniform(0, 2 * np.pi, size=n_hole)
        rings.append(np.stack([cx + r * np.cos(th), cy + r * np.sin(th)], 1))
    euv = np.vstack([rim] + rings)
    # the walls: positions along the rim (outward normals) and the circles (normals towards the hole's axis), below the face
    t = rng.uniform(0, 3.4, size=n_wall // 2)
    wuv = np.where((t < 1.0)[:, None], np.stack([t - 0.5, np.full_like(t, -0.35)], 1),
                   np.where((t < 1.7)[:, None], np.stack([np.full_like(t, 0.5), t - 1.0 - 0.35], 1),
                            np.where((t < 2.7)[:, None], np.stack([2.2 - t, np.full_like(t, 0.35)], 1),
                                     np.stack([np.full_like(t, -0.5), 3.05 - t], 1))))
    wn = np.where((t < 1.0)[:, None], [0.0, -1.0], np.where((t < 1.7)[:, None], [1.0, 0.0], np.where((t < 2.7)[:, None], [0.0, 1.0], [-1.0, 0.0])))
    for cx, cy, r in holes:
        th = rng.uniform(0, 2 * np.pi, size=(n_wall - n_wall // 2) // 3)
        wuv = np.vstack([wuv, np.stack([cx + r * np.cos(th), cy + r * np.sin(th)], 1)])
        wn = np.vstack([wn, np.stack([-np.cos(th), -np.sin(th)], 1)])
    depth = rng.uniform(0.1, 0.9, size=len(wuv)) * thickness
    pts = np.vstack([uv[:, :1] * a + uv[:, 1:] * b, wuv[:, :1] * a + wuv[:, 1:] * b - depth[:, None] * plate_normal])
    nrm = np.vstack([np.tile(tilted, (len(uv), 1)), wn[:, :1] * a + wn[:, 1:] * b])
    ept = euv[:, :1] * a + euv[:, 1:] * b
    ext = np.vstack([pts, ept]).max(axis=0) - np.vstack([pts, ept]).min(axis=0)
    return (np.ascontiguousarray(pts), np.ascontiguousarray(nrm), np.ascontiguousarray(ept), np.tile(tilted, (len(ept), 1)),
            float(np.linalg.norm(ext)))


@functools.lru_cache(maxsize=None)
def estimate_case():
    """the plate posed by T into 1 500 clutter points (sample) and 300 clutter edge points, every fourth of the copy's sample points
    a reference point -> case()'s dict + T"""
    pts, nrm, ept, enr, diameter = plate_with_holes()
    T = pu.pose(3)
    sp, sn, where = pu.scene_of(pts, nrm, T, 1500, 3)
    ep, en, _ = pu.scene_of(ept, enr, T, 300, 53)
    c = _case((pts, nrm, ept, enr), diameter, 0.45 * diameter, params(), (sp, sn, np.sort(where[::4]).astype(np.int64), ep, en))
    c["T"] = T
    return c
