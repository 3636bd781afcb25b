"""A lane carries nothing from one call into the next.

What a segmentation keeps between its rounds -- a RefineModel finished one round late, a tombstone pass waiting to ride in the
next fit's first launch, lists leaving through the copy engine -- and what a fit knows of its queued compaction are values owned
by the call (FitCaller / SegmentRounds / Compaction, m3d_driver_internal.hpp), not members of the lane.  These tests leave a
segmentation at each of its exits and look at the very next calls on the same lane (one thread: lane 0): everything against
the CPU oracle, and the fits on a resident cloud bit for bit against themselves before the segmentation."""
import numpy as np
import pytest

from misc3d_amd import synth

pytestmark = pytest.mark.gpu

PARAM_TOL = 1e-9          # refined parameters against the oracle's serial sums (test_gpu_parity.py)

# Case 1.  room_cloud_c5's planes hold 25 % .. 50 % of the points that are left when their round comes, and poison_fits
# (m3d_segmentation.cpp) lets a round kill its inliers in place only if they are at most a SIXTEENTH of the live points of the
# sorted copy (and the dead stay below an eighth of it): both ratios are free of the cloud's size, so at the threshold of the
# parity tests (0.01: the whole 3 mm-sigma plane) no size makes one of the first rounds a kill.  What decides is the slab:
# at 0.5 mm it holds erf(0.5 / (3 sqrt 2)) = 13 % of a plane, 3.3 % of the cloud for the floor -- every round's removal is a
# sliver.  The size is then the smallest that still has several compaction workgroups (2048 points) and some forty 512-point
# tiles, and is odd: 20 011.  Such a round's fitness (< 0.04) never reaches the adaptive bound, so each fit runs its
# max_iteration = 300 > 2 * lead_hypotheses (128): from round two on the fit gets ONE hinted chunk with RefineModel's
# compaction queued on the device's pick (run_ransac), the round is finished late (deferred) and its kill rides in the next
# round's minimal_fit_k launch; round one, without a hint, kills with a launch of its own.
SEG_N, SEG_THR, SEG_ITERS, SEG_SEED = 20_011, 0.0005, 300, 5
ROUTES = {"default": {}, "no_speculation": {"speculative_refine": 0}}


@pytest.fixture(scope="module")
def room(orc):
    pts = synth.room_cloud_c5(SEG_N, 17)
    ro, po, co = orc.segment_plane_iterative(pts, SEG_THR, max_iteration=SEG_ITERS, seed=SEG_SEED, max_clusters=3)
    assert ro == 0 and len(co) == 3
    alive = SEG_N
    for c in co[:2]:                        # the removals of rounds one and two (round three is the last: none)
        assert 3 <= len(c) and 16 * len(c) <= alive      # poison_fits: a sliver
        alive -= len(c)
    assert 8 * (len(co[0]) + len(co[1])) <= SEG_N          # ... and the dead stay below an eighth
    return pts, po, co


@pytest.fixture(scope="module")
def resident(orc):
    """The other cloud and the oracle's results of the three fits made on it (_fits)."""
    pts = synth.plane_cloud_c1(50_000)
    want = [orc.fit(kind, pts, None, thr=0.01, max_iter=it, prob=prob, seed=seed) for kind, it, prob, seed in FITS]
    return pts, want


# probability 1: the compaction is queued early on the device's pick and ships the list as a bit mask; then the adaptive stop;
# then a sphere
FITS = ((0, 400, 1.0, 11), (0, 1000, 0.9999, 12), (1, 400, 0.9999, 13))


def _fits(cloud):
    return [cloud.fit(kind, 0.01, it, prob, seed=seed) for kind, it, prob, seed in FITS]


def _same_fits(got, before, want):
    for g, b, o in zip(got, before, want):
        assert g.ret == b.ret and np.array_equal(g.inliers, b.inliers)
        assert np.array_equal(g.params.view(np.uint64), b.params.view(np.uint64))
        assert g.stats["best_index"] == b.stats["best_index"] == o.best_index and g.stats["iterations"] == o.iterations
        assert g.ret == o.ret and np.array_equal(g.inliers, o.inliers)
        assert np.allclose(g.params, o.params, rtol=0, atol=PARAM_TOL)


def _segment_cut_short(capi, room, max_clusters):
    pts, po, co = room
    rc, planes, clusters = capi.segment_plane_iterative(pts, SEG_THR, max_iteration=SEG_ITERS, seed=SEG_SEED,
                                                        max_clusters=max_clusters)
    assert rc == 1 and len(clusters) == len(planes) == max_clusters
    for k in range(max_clusters):
        assert np.array_equal(clusters[k], co[k])
        assert np.allclose(planes[k], po[k], rtol=0, atol=PARAM_TOL)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_segmentation_cut_short_by_max_clusters(capi, room, route):
    """Case 1: two clusters, then three, of the same scene: the first call ends with a round whose RefineModel is still to be
    finished and (three clusters) after a round whose kill rode in the last fit; the second call starts where the first
    would have gone on.  Both are the oracle's first two / three."""
    old = capi.set_config(**ROUTES[route])
    try:
        _segment_cut_short(capi, room, 2)
        _segment_cut_short(capi, room, 3)
    finally:
        capi.restore_config(old)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_fits_on_another_cloud_after_each_segmentation(capi, room, resident, route):
    """Case 2: the three fits on a resident cloud, straight after each of case 1's segmentations on the same lane, are what they
    were before it, bit for bit, and the oracle's."""
    pts, want = resident
    old = capi.set_config(**ROUTES[route])
    try:
        with capi.Cloud(pts) as cloud:
            before = _fits(cloud)
            _same_fits(before, before, want)
            for max_clusters in (2, 3):
                _segment_cut_short(capi, room, max_clusters)
                _same_fits(_fits(cloud), before, want)
    finally:
        capi.restore_config(old)


def test_segmentation_that_would_throw_then_fits(capi, orc, resident):
    """Case 3: 600 points of a plane and 2 far off it, min_ratio so small that the target (601) exceeds the plane: round one
    takes the plane, the removal leaves 2 points, and the call ends where the reference's FitModel would throw (return value
    2, one cluster) -- with round one's removal done and nothing after it.  The fits of case 2 follow."""
    rng = np.random.default_rng(23)
    plane = np.c_[rng.uniform(-1, 1, (600, 2)), 0.25 + rng.normal(0, 1e-4, 600)]
    pts = np.concatenate([plane, [[0.3, -0.2, 7.0], [-0.5, 0.4, -6.0]]])[rng.permutation(602)]
    ro, po, co = orc.segment_plane_iterative(pts, 0.01, max_iteration=300, min_ratio=0.001, seed=4)
    assert ro == 2 and len(co) == 1 and len(co[0]) == 600
    rpts, want = resident
    with capi.Cloud(rpts) as cloud:
        before = _fits(cloud)
        rc, planes, clusters = capi.segment_plane_iterative(pts, 0.01, max_iteration=300, min_ratio=0.001, seed=4)
        assert rc == 2 and len(clusters) == 1 and np.array_equal(clusters[0], co[0])
        assert np.allclose(planes, po, rtol=0, atol=PARAM_TOL)
        _same_fits(_fits(cloud), before, want)
