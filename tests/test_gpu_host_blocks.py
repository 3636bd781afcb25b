"""The inlier list in a block of m3d_host_alloc, both ways it gets there: expanded by the host from the device's bit mask
(m3d_config.list_mask 1: spans of the list that begin on 64-byte lines, written by the pool's placed helpers) and written by the
device itself (list_mask 0) -- the same return value, parameters and list at sizes around one and two tiles; and the blocks
themselves: what the registry reports, and that allocating and freeing them leaves the process' mappings where they were."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from misc3d_amd import capi, synth  # noqa: E402


def _plane_points(n):
    """points on z = 0.1 x - 0.2 y + 0.3 with a fifth of clutter, a fixed stream"""
    rng = np.random.default_rng(n)
    p = rng.uniform(-1.0, 1.0, size=(n, 3))
    p[:, 2] = 0.1 * p[:, 0] - 0.2 * p[:, 1] + 0.3 + rng.normal(0.0, 0.002, n)
    clutter = rng.random(n) < 0.2
    p[clutter, 2] = rng.uniform(-1.0, 1.0, int(clutter.sum()))
    return p


def _fit(pts, list_mask):
    old = capi.set_config(list_mask=list_mask)
    try:
        with capi.Cloud(pts) as cloud:
            # copy=False: the list goes into the cloud's own block of m3d_host_alloc
            r = cloud.fit(0, threshold=0.01, max_iteration=300, probability=1.0, seed=5, copy=False)
            return r.ret, r.params.copy(), np.array(r.inliers, copy=True)
    except capi.M3DError as e:   # (a single point: refused the same way both times)
        return e.code, None, None
    finally:
        capi.restore_config(old)


@pytest.mark.parametrize("n", [1, 2047, 2049, 70001])
def test_plane_fit_is_the_same_with_the_mask_and_without(n):
    pts = _plane_points(n)
    ret0, par0, inl0 = _fit(pts, 0)
    ret1, par1, inl1 = _fit(pts, 1)
    assert ret0 == ret1
    if par0 is None or par1 is None:
        assert par0 is None and par1 is None
        return
    assert np.array_equal(par0, par1)
    assert np.array_equal(inl0, inl1)
    if n >= 2047:
        assert len(inl0) > n // 2 and np.all(np.diff(inl0.astype(np.int64)) > 0)


def _host_block(p, nbytes):
    f = capi.lib().m3d_bench_host_block
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_size_t]
    return int(f(p, nbytes))


@pytest.mark.parametrize("nbytes", [4096, 8 << 20])
def test_registry_reports_a_block_inside_its_bounds_only(nbytes):
    L = capi.lib()
    p = L.m3d_host_alloc(nbytes)
    assert p
    try:
        assert _host_block(p, nbytes) == 1
        assert _host_block(p + nbytes - 8, 8) == 1
        assert _host_block(p + 64, nbytes - 64) == 1
        assert _host_block(p, nbytes + 1) == 0
        assert _host_block(p + nbytes, 8) == 0
        assert _host_block(p - 8, 16) == 0
    finally:
        L.m3d_host_free(p)
    assert _host_block(p, 8) == 0
    assert _host_block(p, nbytes) == 0


def _mapped_kb():
    with open("/proc/self/status") as f:
        for line in f:
            if line.startswith("VmSize:"):
                return int(line.split()[1])
    raise RuntimeError("no VmSize")


def test_alloc_free_cycles_leave_the_mapped_size():
    L = capi.lib()
    block = 8 << 20
    for _ in range(3):   # (the runtime's own pools settle)
        L.m3d_host_free(L.m3d_host_alloc(block))
    before = _mapped_kb()
    for _ in range(100):
        p = L.m3d_host_alloc(block)
        assert p
        C.memset(p, 0x5A, 4096)
        L.m3d_host_free(p)
    after = _mapped_kb()
    # one block that stayed mapped per cycle would be 800 MB; a single one 8 MB
    assert after - before < block // 1024, (before, after)


def test_device_writes_the_list_into_a_block_and_the_host_reads_it():
    """list_mask 0: the compaction kernel stores the indices straight into the block; against the CPU oracle"""
    import oracle

    pts = synth.plane_cloud_c1(20000, 1)
    old = capi.set_config(list_mask=0)
    try:
        with capi.Cloud(pts) as cloud:
            r = cloud.fit(0, threshold=0.01, max_iteration=200, probability=0.9999, seed=7, copy=False)
            assert _host_block(r.inliers.ctypes.data, r.inliers.nbytes) == 1
            got = np.array(r.inliers, copy=True)
            ret = r.ret
    finally:
        capi.restore_config(old)
    o = oracle.fit(0, pts, None, thr=0.01, prob=0.9999, max_iter=200, seed=7)
    assert ret == o.ret
    assert np.array_equal(got, o.inliers)
