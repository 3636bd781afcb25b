"""The case tables of the k-NN seam tests, shared by tests/test_gpu_knn_seams.py (the kernels against the restatement) and
tests/test_knn.py (a numpy model with planted faults against the same cases), so that the two cannot drift apart.

A hook case pins the geometry of ONE chunk of the tile path (capi.knn_tile_merge): n rows of dim doubles, m queries, `pages`
pages of kk pairs, S splits of r rows.  The product cases name shapes of m3d_knn_search whose split counts, chunks and pages
follow from the host code (product_geometry / product_chunk restate its two lambdas)."""
import zlib
from collections import namedtuple

import numpy as np

from knn_ref_util import bits

SENT_IDX = 0xFFFFFFFF
SENT_KEY = 0xFFFFFFFFFFFFFFFF
TILE_ROWS, TILE_DIMS, MAX_SPLITS, PAGE_MAX = 32, 16, 256, 128          # m3d_knn.hpp
TILE_CHUNK, GRID_CHUNK, SCRATCH_CAP = 16384, 65536, 256 << 20          # m3d_knn.cpp

HookCase = namedtuple("HookCase", "group family n dim m kk pages S r")


def case_id(c):
    return "%s-%s-n%d-d%d-m%d-k%d-p%d-S%d-r%d" % c


# ---- the hook cases --------------------------------------------------------------------------------------------------
MERGE_S = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
MERGE_R = (1, 3, 33)
MERGE_KK = (1, 17, 128)
MERGE_VARIANTS = ("full", "ragged", "two_empty")


def _merge_n(S, r, variant):
    n = {"full": S * r, "ragged": S * r - (r - 1), "two_empty": (S - 2) * r}[variant]
    return n if n >= 1 else S * r          # S = 1, 2 have no two_empty form: the full one instead


def _merge_cases():
    """Every S meets every r; over its three r it meets each n variant and each kk once ((i + j) % 3 and (i + 2 j) % 3 run
    through 0, 1, 2 with j), and (i, j) -> (i + j, i + 2 j) mod 3 is one-to-one, so every (variant, kk) pair occurs with
    every r somewhere in the table: 13 x 3 geometries x 2 families = 78 calls instead of 702."""
    out = []
    for i, S in enumerate(MERGE_S):
        for j, r in enumerate(MERGE_R):
            variant, kk = MERGE_VARIANTS[(i + j) % 3], MERGE_KK[(i + 2 * j) % 3]
            for family in ("random", "ties"):
                out.append(HookCase("merge", family, _merge_n(S, r, variant), 2, 5, kk, 1, S, r))
    return out


def _hook_cases():
    out = _merge_cases()
    out += [HookCase("qblock", "random", 200, 3, m, 7, 1, 3, 67) for m in (1, 3, 4, 5, 63, 64, 65, 129)]
    out += [HookCase("kcap", "random", 300, 5, 6, kk, 1, 2, 150) for kk in (15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128)]
    out += [HookCase("tile_dim", "random", 100, dim, 6, 7, 1, 2, 50) for dim in (1, 15, 16, 17, 31, 32, 33, 48, 49)]
    out += [HookCase("tile_rows", "random", n, 3, 6, 7, 1, 1, n) for n in (31, 32, 33, 63, 64, 65)]
    out += [HookCase("tile_rows", "random", 4 * 33, 3, 6, 7, 1, 4, 33)]          # splits start off the 32-row tile
    out += [HookCase("pages", "ties", 200, 2, 6, kk, pages, 5, 40) for pages in (2, 3) for kk in (1, 16, 17)]
    for n in (1, 5, 40):
        r = (n + 2) // 3
        out += [HookCase("short", "short", n, 3, 5, kk, pages, 3, r) for pages, kk in ((1, 16), (3, 16), (2, 64))]
    return out


HOOK_CASES = _hook_cases()
assert len(HOOK_CASES) <= 150 and len(set(HOOK_CASES)) == len(HOOK_CASES)


def planted_rows(c):
    """ties family: the first rows of splits 0, 64, 128, 192 and of the last non-empty split and the one 64 below it.  They are
    the only rows at (2, 2, ...), and query 0 sits there: its list begins with equal keys (zero) out of all those splits."""
    last = (c.n - 1) // c.r
    splits = {s for s in (0, 64, 128, 192, last, last - 64) if 0 <= s <= last}
    return sorted(s * c.r for s in splits)


def hook_input(c):
    """-> (data (n, dim), queries (m, dim)), a function of the case alone"""
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    if c.family == "ties":
        data = rng.integers(0, 3, (c.n, c.dim)).astype(np.float64)
        corner = np.all(data == 2.0, axis=1)
        data[corner, 0] = rng.integers(0, 2, int(corner.sum()))            # nobody else at the corner
        data[planted_rows(c)] = 2.0
        q = rng.integers(0, 3, (c.m, c.dim)).astype(np.float64)
        q[0] = 2.0
        return data, q
    return rng.standard_normal((c.n, c.dim)), rng.standard_normal((c.m, c.dim))


def hook_expected(ref, c, data, q):
    """the restatement's first min(pages kk, n) neighbours, then the sentinel -> (indices uint32, key bits uint64)"""
    width = c.pages * c.kk
    ri, _, rd2, _ = ref.search(data, q, width)
    idx = np.full((c.m, width), SENT_IDX, np.uint32)
    key = np.full((c.m, width), SENT_KEY, np.uint64)
    idx[:, :ri.shape[1]] = ri
    key[:, :ri.shape[1]] = bits(rd2)
    return idx, key


def reaches_lane_lists(c, idx, key):
    """does some query's expected list hold equal keys whose rows lie in splits s and s + 64 (one merge lane's two lists)?"""
    for q in range(len(idx)):
        real = idx[q] != SENT_IDX
        split = idx[q][real].astype(np.int64) // c.r
        k = key[q][real]
        for v in np.unique(k):
            s = split[k == v]
            if np.intersect1d(s, s + 64).size:
                return True
    return False


def expects_lane_lists(c):
    """a ties case can reach it: a row exists in split 64 and the list holds the planted rows (at most 6)"""
    return c.family == "ties" and c.group == "merge" and (c.n - 1) // c.r >= 64 and c.kk >= 17


def page_boundary_inside_a_tie(c, key):
    """does a page boundary fall between two equal keys of some query (all of them, for every boundary)?"""
    cuts = [p * c.kk for p in range(1, c.pages)]
    return all(np.any((key[:, cut - 1] == key[:, cut]) & (key[:, cut] != SENT_KEY)) for cut in cuts)


# ---- the product's host choices, restated ----------------------------------------------------------------------------
def product_geometry(n, mc):
    """run_tile's splits_for and what follows it -> (splits launched, rows per split)"""
    qblocks = (mc + 63) // 64
    S = min(MAX_SPLITS, (2048 + qblocks - 1) // qblocks)
    S = max(1, min(S, (n + 511) // 512))
    rps = (n + S - 1) // S
    return (n + rps - 1) // rps, rps


def product_chunk(n, dim, m, kout, page=PAGE_MAX):
    """run_tile's chunk size: 16 384 queries, halved until bytes_for fits the scratch cap"""
    kk_max = min(page, kout)

    def bytes_for(mc):
        qblocks = (mc + 63) // 64
        S = max(1, min(min(MAX_SPLITS, (2048 + qblocks - 1) // qblocks), (n + 511) // 512))
        return mc * (dim * 8 + S * kk_max * 12 + kk_max * 12 + 16)

    mc = min(m, TILE_CHUNK)
    while mc > 1 and bytes_for(mc) > SCRATCH_CAP:
        mc = (mc + 1) // 2
    return mc


def product_tile_launches(n, dim, m, kout, page=PAGE_MAX):
    mc = product_chunk(n, dim, m, kout, page)
    return 2 * ((m + mc - 1) // mc) * ((kout + page - 1) // page)


# the product's own split counts above 64 (8 queries: splits_for gives min(256, ceil(n / 512)))
SPLIT_N = (32768, 32769, 65537, 98305, 130561, 131073)
SPLIT_K = (1, 128)
SPLIT_M = 8


def split_input(n, dim):
    rng = np.random.default_rng(n + dim)
    return rng.integers(0, 256, (n, dim)).astype(np.float64), rng.integers(0, 256, (SPLIT_M, dim)).astype(np.float64)


TILE_CHUNKS = dict(dim=4, n=600, m=TILE_CHUNK + 1)          # k = 3: two chunks; k = 130: two chunks of two pages
HALVING = dict(dim=321, n=3585, m=TILE_CHUNK + 1, k=128)    # 16 408 bytes per query at S = 8: the chunk halves to 8 192
GRID_CHUNKS = dict(dim=3, n=1200, m=GRID_CHUNK + 70)
GRID_CHUNK_NONFINITE = ((100, np.nan), (GRID_CHUNK - 1, np.inf), (GRID_CHUNK, -np.inf))


def chunk_input(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((shape["n"], shape["dim"])), rng.standard_normal((shape["m"], shape["dim"]))


# ---- degenerate density grids ----------------------------------------------------------------------------------------
DEGENERATE_K = (1, 16, 17, 32, 33, 64, 65, 128)
DEGENERATE = ("equal", "line_x", "line_y", "line_z", "plane", "clusters", "n1", "n2", "n3")


def degenerate_rows(name):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name == "equal":
        return np.full((500, 3), 0.375)
    if name.startswith("line_"):
        rows = np.full((1000, 3), -0.5)
        rows[:, "xyz".index(name[-1])] = rng.uniform(-2.0, 3.0, 1000)
        return rows
    if name == "plane":
        rows = rng.uniform(0.0, 1.0, (1000, 3))
        rows[:, 2] = 0.25
        return rows
    if name == "clusters":
        rows = rng.standard_normal((600, 3))
        rows[300:] += 1e12
        return rows
    if name == "nonfinite":
        rows = rng.standard_normal((40, 3))
        bad = rng.permutation(40)[:10]
        for t, i in enumerate(bad):          # five rows with a NaN, five with an infinite coordinate
            rows[i, t % 3] = np.nan if t < 5 else (np.inf, -np.inf)[t % 2]
        return rows
    return rng.standard_normal((int(name[1:]), 3))


def degenerate_queries(rows, count):
    """the box corners, one cell and 1e6 outside each face (a cell: a sixteenth of the longest edge, 1 for a point), then the
    rows themselves up to `count` queries"""
    fin = rows[np.isfinite(rows).all(axis=1)]
    lo, hi = fin.min(axis=0), fin.max(axis=0)
    mid = 0.5 * (lo + hi)
    cell = float((hi - lo).max()) / 16 or 1.0
    q = [[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)]
    for step in (cell, 1e6):
        for a in range(3):
            for side, edge in ((-1.0, lo), (1.0, hi)):
                p = mid.copy()
                p[a] = edge[a] + side * step
                q.append(p)
    q = np.array(q, np.float64)
    own = rows[np.arange(count - len(q)) % len(rows)]
    return np.concatenate([q, own])
