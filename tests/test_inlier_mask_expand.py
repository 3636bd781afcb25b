"""The host half of the inlier-mask form of RefineModel's list (misc3d_amd/csrc/m3d_mask_expand.hpp), CPU only: the header is
compiled on its own with the system compiler and its expansion, portable loop and AVX-512, compared with np.flatnonzero."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR_DIR = os.path.join(ROOT, "misc3d_amd", "csrc")
TILE = 2048

DRIVER = r"""
#include "m3d_mask_expand.hpp"
extern "C" int expand(const uint64_t* mask, uint64_t n, const uint32_t* counts, uint64_t* dst, uint32_t writers, int path) {
    return m3d::mask_expand_threads(mask, n, counts, dst, writers, path) ? 1 : 0;
}
extern "C" int have_avx512() { return m3d::mask_have_avx512() ? 1 : 0; }
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    d = tmp_path_factory.mktemp("mask_expand")
    src = d / "drv.cpp"
    src.write_text(DRIVER)
    so = d / "libdrv.so"
    subprocess.run([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-I", HDR_DIR, str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.expand.restype = C.c_int
    L.expand.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]
    L.have_avx512.restype = C.c_int
    return L


def make_mask(flags):
    """(words, counts) as the device writes them: whole tiles of 32 words, one count per tile of 2048 points"""
    n = len(flags)
    nb = (n + TILE - 1) // TILE
    padded = np.zeros(nb * TILE, dtype=bool)
    padded[:n] = flags
    words = np.packbits(padded, bitorder="little").view(np.uint64).copy()
    counts = padded.reshape(nb, TILE).sum(axis=1).astype(np.uint32) if nb else np.zeros(0, np.uint32)
    return words, counts


def run(lib, flags, writers, path, sentinels=8):
    words, counts = make_mask(flags)
    ref = np.flatnonzero(flags).astype(np.uint64)
    total = len(ref)
    buf = np.full(total + sentinels, 0xDEADBEEFCAFEF00D, dtype=np.uint64)
    ok = lib.expand(words.ctypes.data if len(words) else None, len(flags), counts.ctypes.data if len(counts) else None,
                    buf.ctypes.data, writers, path)
    assert ok == 1
    assert np.array_equal(buf[:total], ref)
    assert np.all(buf[total:] == np.uint64(0xDEADBEEFCAFEF00D)), "a store past the list's end"


def paths(lib):
    return [0, 1] if lib.have_avx512() else [0]


DENSITIES = ["zero", "sparse", "half", "alternate", "ones", "first", "last", "runs"]


def flags_for(kind, n, rng):
    if kind == "zero":
        return np.zeros(n, dtype=bool)
    if kind == "sparse":
        return rng.random(n) < 1e-3
    if kind == "half":
        return rng.random(n) < 0.5
    if kind == "alternate":
        return (np.arange(n) % 2) == 1
    if kind == "ones":
        return np.ones(n, dtype=bool)
    if kind == "first":
        f = np.zeros(n, dtype=bool)
        f[:1] = True
        return f
    if kind == "last":
        f = np.zeros(n, dtype=bool)
        f[-1:] = True
        return f
    # plane-like: long all-ones stretches between clutter
    f = rng.random(n) < 0.03
    for s in range(0, n, 5000):
        f[s:s + 3000] = True
    return f


@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 - 1, 3 * 2048 + 1, 100_003, 1_000_000])
@pytest.mark.parametrize("kind", DENSITIES)
def test_expand_matches_flatnonzero(lib, n, kind):
    rng = np.random.default_rng(n * 31 + len(kind))
    flags = flags_for(kind, n, rng)
    for path in paths(lib):
        for writers in (1, 3, 8):
            run(lib, flags, writers, path)


@pytest.mark.parametrize("writers", list(range(1, 13)))
def test_expand_writers(lib, writers):
    rng = np.random.default_rng(writers)
    flags = flags_for("runs", 300_001, rng)
    for path in paths(lib):
        run(lib, flags, writers, path)


def test_expand_more_writers_than_tiles(lib):
    flags = np.ones(2 * 2048 + 7, dtype=bool)
    for path in paths(lib):
        run(lib, flags, 12, path)


def test_expand_rejects_counts_that_disagree(lib):
    flags = np.zeros(4096, dtype=bool)
    flags[::3] = True
    words, counts = make_mask(flags)
    counts = counts.copy()
    counts[0] -= 1                      # one bit more in tile 0 than its count says
    total = int(counts.sum())
    buf = np.full(total + 8, 7, dtype=np.uint64)
    for path in paths(lib):
        assert lib.expand(words.ctypes.data, len(flags), counts.ctypes.data, buf.ctypes.data, 4, path) == 0
        assert np.all(buf[total:] == 7), "a store past the list's end"
