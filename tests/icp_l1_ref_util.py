"""The restatement of m3d_registration_icp_plane_l1's contract (include/misc3d_amd.h, rules 1 - 8 of the plane call with L1 - L3)
that both L1 test files use.  Nothing here is shared with the library: the search is the grid of tests/cpp/icp_ref.c (built by
icp_ref_util.IcpRef; the moving cloud goes through it under the identity, which leaves finite coordinates as they are), the 27
weighted sums are EXACT sums of the rounded products (math.fsum) -- so no order of summation is preferred over the device's --
or, for the input guard, numpy's pairwise sums over the correspondences in descending order; determinant and solve are numpy's.
The cases are those of icp_ref_util plus one with a residual that is exactly zero."""
import math

import numpy as np

import icp_ref_util as iu

I4 = np.eye(4)


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _apply(T, p):
    """PointCloud::Transform as the contract associates it, ((T0 x + T1 y) + T2 z) + T3 per coordinate: with the weights
    1 / |r| a moved point that differs in its last bit is no small matter (see `case`)"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3] for k in range(3)], axis=1)


def _sum(columns, exact):
    """columns: (m, k) -> k sums over the rows"""
    if exact:
        return np.array([math.fsum(c) for c in columns.T])
    return columns[::-1].sum(axis=0)


def update_l1(s, t, n, exact=True):
    """ComputeTransformation of TransformationEstimationPointToPlane(L1Loss) over the correspondences (s moving, t target, n the
    target's normal): rules 2 - 6 with L1 - L3.  -> (4 x 4 update, solved)"""
    U = np.eye(4)
    if len(s) == 0:
        return U, False
    e = s - t
    r = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = 1.0 / np.abs(r)
        J = np.hstack([np.stack([s[:, 1] * n[:, 2] - s[:, 2] * n[:, 1], s[:, 2] * n[:, 0] - s[:, 0] * n[:, 2],
                                 s[:, 0] * n[:, 1] - s[:, 1] * n[:, 0]], axis=1), n])
        Jw = J * w[:, None]
        terms_A = (Jw[:, :, None] * J[:, None, :]).reshape(len(s), 36)
        terms_b = Jw * r[:, None]
    if not (np.isfinite(terms_A).all() and np.isfinite(terms_b).all()):
        return U, False            # L3: a non-finite record has no finite determinant (rule 5)
    A = _sum(terms_A, exact).reshape(6, 6)
    A = np.triu(A) + np.triu(A, 1).T     # (the record keeps the upper triangle: (J[a] w) J[b] for a <= b)
    b = _sum(terms_b, exact)
    det = np.linalg.det(A)
    if not np.isfinite(det) or abs(det) < 1e-6:
        return U, False
    x = np.linalg.solve(A, -b)
    c, sn = np.cos(x[:3]), np.sin(x[:3])
    Rx = np.array([[1, 0, 0], [0, c[0], -sn[0]], [0, sn[0], c[0]]])
    Ry = np.array([[c[1], 0, sn[1]], [0, 1, 0], [-sn[1], 0, c[1]]])
    Rz = np.array([[c[2], -sn[2], 0], [sn[2], c[2], 0], [0, 0, 1]])
    U[:3, :3], U[:3, 3] = Rz @ Ry @ Rx, x[3:]
    return U, True


def icp_l1(ref, src, dst, max_dist, init, max_iteration, dst_normals, exact=True, rel_fitness=1e-6, rel_rmse=1e-6):
    """RegistrationICP with the L1 estimator.  ref: an icp_ref_util.IcpRef (its search).  -> the dict of IcpRef.icp plus
    `solved`, the number of iterations whose system was solved"""
    src, dst, nrm = _f(src).reshape(-1, 3), _f(dst).reshape(-1, 3), _f(dst_normals).reshape(-1, 3)
    T = I4.copy() if init is None else _f(init).reshape(4, 4).copy()
    mov = src.copy() if np.array_equal(T, I4) else _apply(T, src)

    def result():
        corr = ref.correspondences(mov, dst, max_dist, I4)
        m = corr >= 0
        d = mov[m] - dst[corr[m]]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        c = int(m.sum())
        return corr, c, c / len(src), (math.sqrt(_sum(d2[:, None], exact)[0] / c) if c else 0.0)

    corr, cnt, fit, rm = result()
    it, conv, solved = 0, 0, 0
    while it < max_iteration:
        m = corr >= 0
        U, ok = update_l1(mov[m], dst[corr[m]], nrm[corr[m]], exact)
        solved += int(ok)
        T = U @ T
        if ok:
            mov = _apply(U, mov)
        fit0, rm0 = fit, rm
        corr, cnt, fit, rm = result()
        it += 1
        if abs(fit0 - fit) < rel_fitness and abs(rm0 - rm) < rel_rmse:
            conv = 1
            break
    return {"T": T, "fitness": fit, "inlier_rmse": rm, "correspondences": cnt, "iterations": it, "converged": conv, "corr": corr,
            "solved": solved}


# ("refine" is "no_convergence" with more iterations: it is long_case)
CASES = tuple(n for n in iu.CASES if n != "refine") + ("zero_residual",)
SEAM_SIZES = (255, 256, 257, 16385)


MAX_ITERATION = 3


def case(name):
    """icp_ref_util's case of that name, stopped after MAX_ITERATION iterations at the latest.  The weights 1 / |r| make the
    iteration sensitive to its own roundings: a moved point that differs by 1e-16 changes the weight of a correspondence
    lying 1e-7 from its plane -- among thousands of points with 1e-3 noise there is one -- by 1e-9 of itself, and that weight
    is as large as all the others together.  The difference between two runs so grows by about |update| / min |r| per
    iteration, a factor of 100 to 1000 on these clouds and more on larger ones (on the 6001 points of "refine", summed in two orders:
    4e-14 after two iterations, 1e-10 after four, 3e-5 after twenty-one; tests/test_icp_l1.py prints the last).  A comparison to 1e-9 means something over the first
    iterations only; `long_case` is held to the true pose instead."""
    if name == "zero_residual":
        # no initial pose, so the source is matched as it is; source point 7 IS a target point: r = 0 exactly, w infinite
        c = iu.case("identity_init")
        src = c["src"].copy()
        src[7] = c["dst"][123]
        return dict(c, src=src)
    c = iu.case(name)
    return dict(c, max_iteration=min(c["max_iteration"], MAX_ITERATION))


def seam_case(n):
    """icp_ref_util.sized_case: n moving points; the large one stops an iteration earlier (more points, smaller residuals)"""
    return iu.sized_case(n, max_iteration=MAX_ITERATION if n < 10000 else MAX_ITERATION - 1)


def long_case():
    """thirty iterations allowed: the run ends at the true pose to 1e-3 whatever the roundings"""
    return iu.case("refine")


_cache = {}


def expected(ref, key):
    """the reference result of a case (a name of CASES or a seam size), computed once per session"""
    if key not in _cache:
        c = case(key) if isinstance(key, str) else seam_case(key)
        _cache[key] = (c, icp_l1(ref, c["src"], c["dst"], c["max_dist"], c["init"], c["max_iteration"], c["dst_normals"]))
    return _cache[key]
