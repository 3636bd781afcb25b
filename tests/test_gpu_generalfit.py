"""Refined plane and sphere parameters (RefineModel -> GeneralFit) against the EXACT closed form / least-squares answer of the
fit's own inliers (tests/generalfit_ref_util.py), on every route that produces them and at the seams of the kernels that sum.

The bound:   err(gpu) <= max(M err(oracle), F),   F = 16 * 2^-53 * max(1, max |inlier coordinate|, max |exact parameter|)
err = the largest absolute parameter error against the exact answer; err(oracle) is the fp64 oracle's own.  M is set by
measurement against the oracle's error, never against the code under test: a power of two at least 4 x above the largest
ratio err / max(err(oracle), F) measured below, and at least 4 x below what the arithmetic with the sums' provisional centre at
the minimal sphere's CENTRE gives on the 10 and 5 degree caps (tests/test_generalfit.py: 732 and 799).  M = 32.

MEASURED on an MI355X: err / max(err(oracle), F); every fused route of a family gives the same bits; "2p" = the two-pass
sums of Cloud.refine:
  family                    err(oracle)   fused    2p     | parent (sums about the minimal sphere's centre), fused
  sphere_full                 8.3e-15      0.01    0.03   |   0.00
  sphere_cap20                4.8e-15      0.03    0.04   |   0.11
  sphere_cap10                2.6e-15      3.82    2.14   |   1747.60   FAILS the bound
  sphere_cap5_r5              1.0e-14      2.29    7.91   |   680.18    FAILS the bound
  sphere_cap10_at_1e3         2.1e-08      0.00    0.00   |   0.00
  sphere_cap5_r5_at_1e3       1.1e-09      0.00    0.00   |   0.06
  sphere_cap10_at_1e5         1.0e-04       -      0.00   |    -        (no RANSAC fit exists: Case.ransac)
  sphere_cap5_r5_at_1e5       4.4e-06       -      0.00   |    -
  sphere_r1mm                 2.3e-18      0.00    0.00   |   0.00
  sphere_4_inliers            3.8e-15      0.25    0.61   |   89.68     FAILS the bound (F: the oracle's error is below it)
  sphere_5_inliers            5.2e-16      0.08    0.03   |   0.03
  sphere_6_inliers            1.9e-16      0.03    0.17   |   0.02
  plane_tilt                  1.1e-15      0.03    0.01
  plane_tilt_at_1e4           1.6e-11      0.09    0.01
  plane_tilt_at_1e6           6.7e-10      0.05    0.05
  plane_strip_100x0.1         5.6e-15      0.01    0.02
  plane_near_collinear        1.0e-16      0.03    0.02
  plane_tie_110 / _1m10       6e-16        0.14 / 0.15   0.04 / 0.03      (undecided: against the nearer branch, modulo sign)
  plane_3_inliers / _4        2e-16/6e-17  0.30 / 0.09   0.12 / 0.03
  plane_cluster_norm_above    4.2e-16      0.05    0.05      (norm_below: GeneralFit fails, the minimal model bit for bit)
  room, three planes          <= 2.4e-15   0.01, 0.02, 0.02
  seams (42 clouds)           plane <= 0.06, sphere <= 0.64
Largest ratio 7.91 (an unchanged path: the two-pass sums on the 5 degree cap), 4 x 7.91 = 31.6 <= M = 32 <= 680 / 4.
The parent passes the translated caps and the 20 degree cap: there the oracle -- Householder QR of the uncentred system -- is
itself 1e-9 .. 2e-8 off, resp. the loss (radius / extent)^3 = 27 is the oracle's own size; the bound is relative to it.
One-edit mutants, run once against this file: the fold's stride 64 -> 63 (fold_moment_partials; scan_blocks_k's own fold
is not launched with partials any more): seams from 64 tiles on and the stale-partials test; partial row * 16 -> * 12: every
fused route of more than one tile, the room, seams from 2049 on; sum_moments_k's mean / (n - 1): the two-pass route, 20 of 23
families; c0 back to the centre: the three families above; centred[1] with m[0] * m[2] and the 2.0 * Sm[k] factor dropped:
tests/test_generalfit.py::test_closed_forms_on_exact_moments on the CPU (ratios 1e11 and 1e14).
"""
import numpy as np
import pytest

import generalfit_ref_util as gu

pytestmark = pytest.mark.gpu

RANSAC_FAMILIES = [n for n in gu.FAMILIES if "_at_1e5" not in n]
M = gu.M_BOUND


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _kw(case):
    return dict(threshold=case.thr, max_iteration=case.max_iter, probability=case.prob, seed=case.seed)


def _exact_parts(g, p, what):
    """what the suite already holds bit for bit: the return value, the winner, the counters, the inlier list"""
    o = p.fit
    st = g.stats
    assert (g.ret, st["best_index"], st["count"], st["iterations"], st["general_fit_ok"]) == \
        (o.ret, o.best_index, o.count, o.iterations, o.general_fit_ok), what
    assert np.array_equal(g.inliers, o.inliers), what


def _refined(params, p, what, ok=1):
    """the bound (or, where the exact closed form fails, the minimal model bit for bit); -> the measured ratio"""
    if not p.exact["ok"]:
        assert ok == 0 and np.array_equal(_bits(params), _bits(p.minimal[:4])), what
        print(f"{what}: the closed form fails exactly -> the minimal model, bit for bit")
        return None
    assert ok == 1, what
    e = gu.err_case(p.case.kind, params, p.exact)
    r = e / max(p.oracle_err, p.F)
    print(f"{what}: err {e:.3e}  err(oracle) {p.oracle_err:.3e}  F {p.F:.3e}  ratio {r:.2f}")
    assert e <= p.bound, (what, e, p.bound, r)
    return r


@pytest.mark.parametrize("name", RANSAC_FAMILIES)
def test_family_on_every_fused_route(capi, orc, name):
    """the one-call fit, two fits on a resident cloud, the batch, and the fits with speculative_refine = 0 and mask_early = 0:
    exact parts against the oracle, the parameters against the exact answer of the fit's own inliers.  All of them fold the
    same per-tile partials in the same order (compact_count_k<.., true> / the moments riding in compact_write_k, then
    scan_blocks_k's order): bit-identical parameters."""
    p = gu.prepare(name, orc)
    case, k = p.case, p.case.kind
    assert case.ransac and (p.exact["ok"] or name in gu.FAIL_FAMILIES)
    if k == gu.PLANE:       # undecided cases occur in the tie families and nowhere else
        assert (p.exact["gap"] < gu.UNDECIDED_GAP) == (name in gu.TIE_FAMILIES)
    fits = [("one-call", capi.fit(k, case.pts, **_kw(case)))]
    with capi.Cloud(case.pts) as c:
        fits.append(("resident #1", c.fit(k, **_kw(case))))
        fits.append(("resident #2", c.fit(k, **_kw(case))))
        fits.append(("batch", capi.fit_batch([(c, k, case.thr, case.max_iter, case.prob, case.seed)])[0]))
        for knob in ("speculative_refine", "mask_early"):
            old = capi.set_config(**{knob: 0})
            try:
                fits.append((knob + "=0 one-call", capi.fit(k, case.pts, **_kw(case))))
                fits.append((knob + "=0 resident", c.fit(k, **_kw(case))))
            finally:
                capi.restore_config(old)
    for what, g in fits:
        _exact_parts(g, p, f"{name} {what}")
        _refined(g.params, p, f"{name} {what}", g.stats["general_fit_ok"])
    for what, g in fits[1:]:
        assert np.array_equal(_bits(g.params), _bits(fits[0][1].params)), (name, what)


@pytest.mark.parametrize("name", list(gu.FAMILIES))
def test_family_on_the_two_pass_route(capi, orc, name):
    """Cloud.refine on the winning minimal model (on the true model where no RANSAC fit exists): sum_xyz_k + sum_moments_k +
    general_fit_sums_finish, with the inlier count known in advance and unknown -- the same launches on the same list"""
    p = gu.prepare(name, orc)
    case, k = p.case, p.case.kind
    start = p.minimal[:4] if case.ransac else case.model
    with capi.Cloud(case.pts) as c:
        rc_u, par_u, inl_u = c.refine(k, case.thr, start)
        rc_e, par_e, inl_e = c.refine(k, case.thr, start, expected=len(p.inliers))
    assert np.array_equal(inl_u.astype(np.int64), p.inliers) and np.array_equal(inl_e.astype(np.int64), p.inliers)
    assert rc_u == rc_e == p.oracle_ok and np.array_equal(_bits(par_u), _bits(par_e))
    if not p.exact["ok"]:
        assert rc_u == 0 and np.array_equal(_bits(par_u), _bits(start))
    else:
        _refined(par_u, p, f"{name} 2p", rc_u)


def test_segmentation_planes_against_the_exact_fit_of_their_clusters(capi, orc):
    """segment_plane_iterative on a three-plane room of 6000 points: every round's GeneralFit is the deferred one
    (finalize_deferred_refine) -- each plane against the exact closed form of its own cluster"""
    pts = gu.room()
    assert len(pts) == 6000
    rc_o, planes_o, clusters_o = orc.segment_plane_iterative(pts, 0.01, max_iteration=100, min_ratio=0.3, seed=3)
    rc, planes, clusters = capi.segment_plane_iterative(pts, 0.01, max_iteration=100, min_ratio=0.3, seed=3)
    assert len(planes) == len(planes_o) == 3 and all(len(c) > 1000 for c in clusters)
    for i, (cl, cl_o) in enumerate(zip(clusters, clusters_o)):
        assert np.array_equal(cl, cl_o)
        inl = pts[cl.astype(np.int64)]
        ex = gu.exact_plane(inl)
        assert ex["ok"] and ex["gap"] >= gu.UNDECIDED_GAP
        F = gu.floor_F(inl, ex["params"])
        e_o, e = gu.err(planes_o[i], ex["params"]), gu.err(planes[i], ex["params"])
        print(f"room plane {i} ({len(cl)} points): err {e:.3e}  err(oracle) {e_o:.3e}  F {F:.3e}  ratio {e / max(e_o, F):.2f}")
        assert e <= max(M * e_o, F)


# ---------------------------------------------------------------------------------------------- seams
_SEAM_EXACT = {}


def _seam_exact(kind, pts, idx):
    """one exact answer per kind: every seam cloud carries the same SET of structure points"""
    if kind not in _SEAM_EXACT:
        inl = pts[idx]
        ex = gu.exact(kind, inl)
        _SEAM_EXACT[kind] = (ex, gu.floor_F(inl, ex["params"]), inl[np.lexsort(inl.T)])
    return _SEAM_EXACT[kind]


def _seam_check(capi, orc, kind, case, fit, what):
    o = orc.fit(kind, case.pts, None, thr=case.thr, max_iter=case.max_iter, prob=case.prob, seed=case.seed)
    g = fit(case)
    assert (g.ret, g.stats["best_index"], g.stats["count"], g.stats["iterations"], g.stats["general_fit_ok"]) == \
        (o.ret, o.best_index, o.count, o.iterations, 1), what
    assert np.array_equal(g.inliers, o.inliers) and np.array_equal(g.inliers.astype(np.int64), case.structure), what
    ex, F, key = _seam_exact(kind, case.pts, case.structure)
    inl = case.pts[case.structure]
    assert np.array_equal(inl[np.lexsort(inl.T)], key)      # the same set
    e_o, e = gu.err(o.params, ex["params"]), gu.err(g.params, ex["params"])
    print(f"{what}: err {e:.3e}  err(oracle) {e_o:.3e}  F {F:.3e}  ratio {e / max(e_o, F):.2f}")
    assert e <= max(M * e_o, F), (what, e, e_o, F)
    return g


@pytest.mark.parametrize("n", gu.SEAM_SIZES)
@pytest.mark.parametrize("kind", [gu.PLANE, gu.SPHERE])
def test_seams_of_the_fused_sums(capi, orc, kind, n):
    """cloud sizes around one tile of kCompactTile points, around the 64-wide stride of the fold of the tiles' partials and
    beyond 1024 tiles; 2000 inliers spread over the whole index range, only in the last tile, only in tile 0 (but for
    hypothesis 0's sample points, which lie where the sampler looks), everything else far outliers"""
    for layout in gu.SEAM_LAYOUTS:
        case = gu.seam_case(kind, n, layout, orc)
        assert len(case.pts) == n and len(case.structure) == gu.SEAM_INLIERS
        rest = np.setdiff1d(case.structure, orc.draw_samples(n, 3 + kind, 1, case.seed)[0].astype(np.int64))
        if layout == "tile_0":
            assert rest.max() < gu.K_TILE
        elif layout == "last_tile":
            assert rest.min() >= n - gu.K_TILE
        _seam_check(capi, orc, kind, case, lambda c: capi.fit(kind, c.pts, **_kw(c)), case.name)


@pytest.mark.parametrize("kind", [gu.PLANE, gu.SPHERE])
def test_small_fit_after_a_large_one_reads_no_stale_partials(capi, orc, kind):
    """65 tiles of partials, then a fit of one tile on the same context (the calling thread's: one-call fits; a resident
    cloud's lane): the small fit's parameters are those it gives on its own, bit for bit"""
    big = gu.seam_case(kind, 65 * gu.K_TILE, "spread", orc)
    small = gu.seam_case(kind, 2047, "spread", orc)
    one = lambda c: capi.fit(kind, c.pts, **_kw(c))
    first = _seam_check(capi, orc, kind, small, one, small.name + " alone")
    _seam_check(capi, orc, kind, big, one, big.name)
    again = _seam_check(capi, orc, kind, small, one, small.name + " after the large fit")
    assert np.array_equal(_bits(first.params), _bits(again.params))
    with capi.Cloud(big.pts) as cb, capi.Cloud(small.pts) as cs:
        _seam_check(capi, orc, kind, big, lambda c: cb.fit(kind, **_kw(c)), big.name + " resident")
        res = _seam_check(capi, orc, kind, small, lambda c: cs.fit(kind, **_kw(c)), small.name + " resident, after the large fit")
    assert np.array_equal(_bits(first.params), _bits(res.params))
