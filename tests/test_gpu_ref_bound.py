"""The planes' reference-histogram bound (m3d_ref_hist.hpp ref_hist_tile, m3d_bound_fp.hpp ref_pair_ub, plane_bound_k) on the device.

m3d_config.ref_bound = 2 forces it at any size.  It may only ever drop hypotheses the sequential loop could not have noticed: every
fit is the oracle's and the fit of ref_bound = 0, every record is that of ref_bound = 0 or 0, and the sums of the bound alone
(m3d_bench_plane_ref_upper_bounds) are upper bounds of the exact counts, hypothesis by hypothesis.  Shapes: the smallest at which
each seam exists -- 6 tiles with a NaN-padded last one under a lead of 128 and two more groups; 40 tiles under 4096 hypotheses.
"""
import numpy as np
import pytest

from misc3d_amd import synth

pytestmark = pytest.mark.gpu

THR = 0.01
CASES = ["small", "dominant", "parallel", "far", "clutter", "degenerate_lead"]
SEED = {"small": 3, "dominant": 5, "parallel": 7, "far": 9, "clutter": 11, "degenerate_lead": 13}


def _cloud(case, capi):
    """-> (points, hypotheses)"""
    rng = np.random.default_rng(41)
    if case == "small":                # 3000 points: 6 tiles, the last one padded with NaN; lead 128 + two groups
        return synth.plane_cloud_c2(3000, 2), 256
    n, H = 20_000, 4096
    if case == "dominant":
        pts = synth.plane_cloud_c2(n, 2)
    elif case == "parallel":           # two parallel planes 5 cut-offs apart: both inside the histogram's span
        nrm = np.array([0.3, -0.2, 0.93]) / np.linalg.norm([0.3, -0.2, 0.93])
        a = np.cross(nrm, [1.0, 0.0, 0.0])
        a /= np.linalg.norm(a)
        b = np.cross(nrm, a)
        uv = rng.uniform(-2, 2, size=(n, 2))
        h = np.where(np.arange(n) < 0.45 * n, 0.0, 5 * THR) + 0.003 * rng.normal(size=n)
        pts = uv[:, :1] * a + uv[:, 1:] * b + h[:, None] * nrm
        pts[int(0.8 * n):] = rng.uniform(-2, 2, size=(n - int(0.8 * n), 3))
        pts = pts[rng.permutation(n)]
    elif case == "far":                # 300 scene sizes (4) from the origin
        pts = synth.plane_cloud_c2(n, 3) + np.array([1200.0, -900.0, 600.0])
    elif case == "clutter":            # the lead finds nothing good
        pts = rng.uniform(-2, 2, size=(n, 3))
    else:                              # every one of the leading 128 hypotheses is degenerate: its three points coincide
        pts = synth.plane_cloud_c2(n, 4)
        lead = capi.draw_samples(n, 0, 128, SEED[case]).reshape(-1)
        pts[lead] = pts[lead[0]]
    return np.ascontiguousarray(pts), H


@pytest.fixture(scope="module")
def clouds(capi):
    return {case: _cloud(case, capi) for case in CASES}


def _fit_and_records(capi, pts, H, seed, **cfg):
    old = capi.set_config(**cfg)
    try:
        with capi.Cloud(pts) as c:
            g = c.fit(0, THR, H, 1.0, seed=seed)
            sm = c.make_sampler(0, seed)
            try:
                rec = c.score_shard_packed(sm, THR, 0, H, H, 1, 0)   # one rank, from hypothesis 0: a fit's first chunk
            finally:
                sm.close()
    finally:
        capi.restore_config(old)
    return g, rec


@pytest.mark.parametrize("case", CASES)
def test_fits_and_records_are_identical_with_the_reference_bound(capi, orc, clouds, case):
    pts, H = clouds[case]
    seed = SEED[case]
    o = orc.fit(0, pts, None, thr=THR, max_iter=H, prob=1.0, seed=seed, lookahead=128)
    g0, r0 = _fit_and_records(capi, pts, H, seed, ref_bound=0)
    g2, r2 = _fit_and_records(capi, pts, H, seed, ref_bound=2)
    for g in (g0, g2):
        assert (g.ret, g.stats["best_index"], g.stats["count"]) == (o.ret, o.best_index, o.count)
        assert np.array_equal(g.inliers, o.inliers)
    assert g2.ret == g0.ret and np.array_equal(g2.params, g0.params)
    assert np.allclose(g2.params, o.params, rtol=0, atol=1e-9 * max(1.0, float(np.abs(o.params).max())))   # (order-free GeneralFit sums)
    assert len(r0) == len(r2) == H
    assert np.all((r2 == r0) | ((r2 & 0x7FFFFFFF) == 0)), np.nonzero((r2 != r0) & ((r2 & 0x7FFFFFFF) != 0))[0][:5]
    assert np.array_equal(r2 >> 31, r0 >> 31)
    if o.best_index >= 0:
        assert r2[o.best_index] == r0[o.best_index]
    # the bound is the smaller of two: on a cloud with a plane to find it spares work the frames' bound alone does not
    gp, _ = _fit_and_records(capi, pts, H, seed, ref_bound=0, plane_bound=2)
    print(case, "pairs scored: bound off", g0.stats["pairs_scored"], "frames' bound", gp.stats["pairs_scored"], "+ reference", g2.stats["pairs_scored"])
    if case in ("dominant", "parallel", "far"):   # (without structure nothing is pruned, and the count varies by a few pairs from run to run)
        assert g2.stats["pairs_scored"] < gp.stats["pairs_scored"]


@pytest.mark.parametrize("case", CASES)
def test_reference_sums_are_upper_bounds(capi, clouds, case):
    """ref_pair_ub alone, summed per hypothesis over the touched tiles, against the exact counts -- the reference being what a fit
    takes (the best of the leading 128 hypotheses), or the table's best where none of those is valid."""
    pts, H = clouds[case]
    samples = capi.draw_samples(len(pts), 0, H, SEED[case])
    with capi.Cloud(pts) as c:
        val, _, cnt = c.score_range(0, THR, samples, 0, H, want_models=False)
        cnt = np.where(val.astype(bool), cnt.astype(np.int64), -1)
        ref = int(np.argmax(cnt[:128])) if cnt[:128].max() > 0 else int(np.argmax(cnt))
        ub = c.plane_ref_upper_bounds(THR, samples, ref).astype(np.int64)
    bad = np.nonzero(ub < cnt)[0]
    assert len(bad) == 0, (case, ref, bad[:5], ub[bad[:5]], cnt[bad[:5]])
    print(case, "reference", ref, "count", int(cnt[ref]), "its own bound", int(ub[ref]))
    if case in ("dominant", "far", "parallel"):   # the reference bounds itself within a bin's worth of points per tile
        assert ub[ref] - cnt[ref] < 0.15 * cnt[ref] + 64, (int(ub[ref]), int(cnt[ref]))
