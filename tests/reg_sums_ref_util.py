"""The registration sums (m3d_reg_kernels.hip: umeyama_sums_k over the pairs of m3d_kabsch and over an ICP step's correspondences
-- recorded under the keys "kabsch_sums_k" and "icp_sums_k" --, icp_err_k, info_sums_k + kabsch_final_k) restated:
an exact reference, the error bound their summation shape implies, a numpy emulation of that shape with the mutations the
tests must notice, and the input families of tests/test_reg_sums.py (CPU) and tests/test_gpu_reg_sums.py.

THE SUMS.  For m correspondences (s_i, d_i) out of n rows the kernels return
    pass 0    S_k = sum s_ik, D_k = sum d_ik                                  (6 values, terms = the inputs: 0 roundings each)
    pass 1    C_rc = sum (d_ir - md_r)(s_ic - ms_c), V_c = sum (s_ic - ms_c)^2   (12 values, 3 roundings per term: two
              centring subtractions and the product), with the kernels' own means ms = fl(S * fl(1 / m)), md likewise
    error     E = sum d2_i, count = sum 1                                     (d2_i as icp_nn_k stored it: 0 roundings)
    moments   sum x, y, z (0 roundings), sum xx, yy, zz, xy, xz, yz (1) over the matched target points
(m_kabsch: m = n, every row a correspondence).

THE EXACT REFERENCE does the same in integer arithmetic: every double is an integer times a power of two (np.frexp), sums and
sums of products of Python integers are exact, and the centred sums are taken about the EXACT means S / m:
    C_rc = sum (m d_ir - D_r)(m s_ic - S_c) / m^2
so is sum |t_i| of every quantity.  One rounding at the very end (float(Fraction) rounds correctly).

THE BOUND.  Every kernel runs <<<256, 256>>> with i += 65536: a thread adds its L = ceil(n / 65536) terms serially, a 256-leaf
tree in LDS (8 levels) makes the block's record, a second 256-leaf tree (8 levels, kabsch_final_k) adds the 256 records.  A
term therefore passes through at most D = L + 16 additions, each of relative error <= u = 2^-53, after its own r <= 3 roundings:
    |computed - sum t^_i| <= ((1 + u)^(D + r) - 1) sum |t^_i|  =  (D + r) u sum |t^_i| + O(u^2)
where t^_i are the terms about the kernels' ROUNDED means m^ = m + dm.  Expanding,
    sum (d_i - md - dmd)(s_i - ms - dms) = sum t_i - dms sum (d_i - md) - dmd sum (s_i - ms) + m dmd dms
and the two cross terms vanish exactly (deviations from the exact mean sum to zero), so centring about a rounded mean adds
m |dmd| |dms| and nothing of first order; sum |t^_i| differs from sum |t_i| by terms of order dm, i.e. second order.  The mean
errors come from the pass-0 sums in the same way, plus TWO roundings: fl(1 / m) and the product (1 / m is exact only for powers
of two):
    |dm| <= (D u sum |x_i| + 2 u |sum x_i|) / m.
Together, first order:
    |got - exact| <= (D + r) u sum |t_i| + m |dm_d| |dm_s|,
and the tests allow exactly twice that for everything of second order -- no measured constant anywhere.  What the public API
derives from the sums gets its own roundings added to the first-order expression before the factor 2 (derived_*): one rounding
for yy + zz, the division and the square root for rmse = sqrt(E / count).

On the exact-integer families (|x| <= 2^10, coordinate sums exactly 0) every partial sum in any order is an integer below 2^53
and every mean is exactly 0: the kernels must return the reference bit for bit there, which is what pins the INDEXING of the
reduction (a skipped index, a dropped trip, a record too few in the final tree); the bound pins its arithmetic.
"""
import decimal
import functools
import math
from fractions import Fraction

import numpy as np

import icp_ref_util as iu

U = Fraction(1, 2 ** 53)
STRIDE = 65536            # 256 blocks x 256 threads

KABSCH_SIZES = (3, 4, 255, 256, 257, 65535, 65536, 65537, 131073)
ICP_SIZES = (1, 255, 256, 257, 65535, 65536, 65537, 131073)
PROBE_POSITIONS = (0, 255, 256, 65535, 65536, 65537, -1)
MASKS = ("all", "none", "ge65536", "last", "every_second")

# roundings a term carries before it is added: the 18 Kabsch sums, (error, count), the 9 moments
R_KABSCH = (0,) * 6 + (3,) * 12
R_ERR = (0, 0)
R_INFO = (0, 0, 0, 1, 1, 1, 1, 1, 1)


def depth(n):
    """additions a term passes through: ceil(n / 65536) serial ones, 8 + 8 tree levels"""
    return -(-int(n) // STRIDE) + 16


# ---------------------------------------------------------------------------------------------- exact arithmetic
def _ints(col):
    """finite doubles -> (object array X of Python ints, E) with col[i] == X[i] * 2^E exactly"""
    col = np.ascontiguousarray(col, dtype=np.float64)
    assert np.isfinite(col).all()
    m, e = np.frexp(col)
    M = np.ldexp(m, 53).astype(np.int64)
    nz = M != 0
    if not nz.any():
        return np.zeros(len(col), dtype=object), 0
    E = e.astype(np.int64) - 53
    emin = int(E[nz].min())
    sh = np.where(nz, E - emin, 0)
    X = np.array([a << b for a, b in zip(M.tolist(), sh.tolist())], dtype=object)
    return X, emin


def _isum(X):
    return sum(X.tolist()) if len(X) else 0


def _scale(v, e):
    return Fraction(v) * (Fraction(2) ** e)


class Exact:
    """values: exact Fractions; abs: exact sum |t_i| per value; extra: the first-order term beside (D + r) u abs (Fractions);
    nan: positions the kernels must return NaN at"""

    def __init__(self, values, abs_, roundings, n_loop, extra=None, nan=None):
        self.values, self.abs, self.r, self.n_loop = list(values), list(abs_), tuple(roundings), int(n_loop)
        self.extra = list(extra) if extra is not None else [Fraction(0)] * len(self.values)
        self.nan = list(nan) if nan is not None else [False] * len(self.values)

    def rounded(self):
        return np.array([float("nan") if z else float(v) for v, z in zip(self.values, self.nan)])

    def first_order(self, k):
        return (depth(self.n_loop) + self.r[k]) * U * self.abs[k] + self.extra[k]

    def bound(self, k):
        return 2 * self.first_order(k)

    def ratios(self, got):
        """|got - exact| / bound per value (0 where both are 0, inf where the bound is 0 and the value differs); NaN
        positions must be NaN (ratio 0) and no other position may be"""
        out = []
        for k, g in enumerate(np.asarray(got, dtype=np.float64).tolist()):
            if self.nan[k]:
                out.append(0.0 if math.isnan(g) else math.inf)
                continue
            if not math.isfinite(g):
                out.append(math.inf)
                continue
            err, b = abs(Fraction(g) - self.values[k]), self.bound(k)
            out.append(0.0 if err == 0 else (math.inf if b == 0 else float(err / b)))
        return out


def exact_pairs(s, d, n_loop):
    """the 18 Kabsch sums over the correspondences (s_i, d_i) (m x 3 each), the loop having run over n_loop rows.  Columns that
    hold a NaN make the sums they enter NaN (and, through the mean, every centred sum of their side's column)."""
    s, d = np.asarray(s, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    m = len(s)
    if m == 0:
        return Exact([Fraction(0)] * 18, [Fraction(0)] * 18, R_KABSCH, n_loop)
    bad_s, bad_d = ~np.isfinite(s).all(axis=0), ~np.isfinite(d).all(axis=0)
    s, d = np.where(np.isfinite(s), s, 0.0), np.where(np.isfinite(d), d, 0.0)
    cols = [_ints(s[:, k]) for k in range(3)] + [_ints(d[:, k]) for k in range(3)]
    tot = [_isum(X) for X, _ in cols]
    values = [_scale(t, e) for t, (_, e) in zip(tot, cols)]
    abs_ = [_scale(_isum(np.abs(X)), e) for X, e in cols]
    Dp = depth(n_loop)
    dm = [(Dp * U * a + 2 * U * abs(v)) / m for v, a in zip(values, abs_)]   # |error of the kernels' mean|
    Y = [X * m - t for (X, _), t in zip(cols, tot)]                          # m x_i - sum x: the centred value times m
    extra = [Fraction(0)] * 6
    for r in range(3):
        for c in range(3):
            P = Y[3 + r] * Y[c]
            e = cols[3 + r][1] + cols[c][1]
            values.append(_scale(_isum(P), e) / (m * m))
            abs_.append(_scale(_isum(np.abs(P)), e) / (m * m))
            extra.append(m * dm[3 + r] * dm[c])
    for c in range(3):
        P = Y[c] * Y[c]
        e = 2 * cols[c][1]
        values.append(_scale(_isum(P), e) / (m * m))
        abs_.append(values[-1])
        extra.append(m * dm[c] * dm[c])
    nan = list(bad_s) + list(bad_d) + [bool(bad_d[r] or bad_s[c]) for r in range(3) for c in range(3)] + list(bad_s)
    return Exact(values, abs_, R_KABSCH, n_loop, extra, nan)


def exact_kabsch(src, dst):
    return exact_pairs(src, dst, len(np.asarray(src).reshape(-1, 3)))


def exact_column_sum(x):
    """-> (sum x_i, sum |x_i|), exact"""
    X, e = _ints(x)
    return _scale(_isum(X), e), _scale(_isum(np.abs(X)), e)


def exact_moments(t, n_loop):
    """the 9 moments of the matched target points t (m x 3)"""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    if len(t) == 0:
        return Exact([Fraction(0)] * 9, [Fraction(0)] * 9, R_INFO, n_loop)
    cols = [_ints(t[:, k]) for k in range(3)]
    values = [_scale(_isum(X), e) for X, e in cols]
    abs_ = [_scale(_isum(np.abs(X)), e) for X, e in cols]
    for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)):
        P = cols[a][0] * cols[b][0]
        e = cols[a][1] + cols[b][1]
        values.append(_scale(_isum(P), e))
        abs_.append(_scale(_isum(np.abs(P)), e))
    return Exact(values, abs_, R_INFO, n_loop)


# ---------------------------------------------------------------------------------------------- the ICP step's reference
def move(src, T):
    """icp_transform_k: ((t0 x + t1 y) + t2 z) + t3 per row of T"""
    src, T = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(T, dtype=np.float64).reshape(4, 4)
    x, y, z = src[:, 0], src[:, 1], src[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def brute_correspondences(moved, dst, max_dist):
    """nearest target point of every moved point by exhaustive search: d2 = (dx dx + dy dy) + dz dz as the kernels form it, the
    lowest index on ties, a correspondence iff d2 < max_dist * max_dist -> (corr int64 or -1, d2 with 0 where unmatched)"""
    moved, dst = np.asarray(moved, dtype=np.float64).reshape(-1, 3), np.asarray(dst, dtype=np.float64).reshape(-1, 3)
    r2 = float(max_dist) * float(max_dist)
    n = len(moved)
    corr, d2s = np.full(n, -1, dtype=np.int64), np.zeros(n)
    if n == 0 or len(dst) == 0:
        return corr, d2s
    step = max(1, (1 << 22) // len(dst))
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(0, n, step):
            p = moved[b:b + step]
            dx, dy, dz = (p[:, None, k] - dst[None, :, k] for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            d2 = np.where(np.isnan(d2), np.inf, d2)
            k = np.argmin(d2, axis=1)                 # the first minimum: lowest index on ties
            best = d2[np.arange(len(p)), k]
            ok = best < r2
            corr[b:b + step] = np.where(ok, k, -1)
            d2s[b:b + step] = np.where(ok, best, 0.0)
    return corr, d2s


class IcpExact:
    """one evaluation of the point-to-point step, exactly: corr, count, err (Exact of 2), sums (Exact of 18), info (Exact of 9)"""

    def __init__(self, src, dst, max_dist, T):
        src, dst = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(dst, dtype=np.float64).reshape(-1, 3)
        n = len(src)
        self.moved = move(src, T)
        self.corr, self.d2 = brute_correspondences(self.moved, dst, max_dist)
        m = self.corr >= 0
        self.matched, self.count, self.n = m, int(m.sum()), n
        e, ea = exact_column_sum(self.d2[m])
        self.err = Exact([e, Fraction(self.count)], [ea, Fraction(self.count)], R_ERR, n)
        self.s, self.d = self.moved[m], dst[self.corr[m]]
        self.sums = exact_pairs(self.s, self.d, n)
        self.info = exact_moments(self.d, n)

    def rounded(self):
        return np.concatenate([self.err.rounded(), self.sums.rounded(), self.info.rounded()])

    def ratios(self, out):
        """per kernel: the largest |got - exact| / bound of m3d_bench_icp_sums' 29 outputs"""
        return {"icp_err_k": max(self.err.ratios(out[0:2])), "icp_sums_k": max(self.sums.ratios(out[2:20])),
                "info_sums_k": max(self.info.ratios(out[20:29]))}


# ---- what the public API derives from the sums: (exact value, bound) with the extra roundings in the first-order expression
def derived_sum2(ex, a, b):
    """fl(v_a + v_b), e.g. info[0, 0] = yy + zz: one more rounding"""
    v = ex.values[a] + ex.values[b]
    return v, 2 * (ex.first_order(a) + ex.first_order(b) + U * abs(v))


def derived_rmse(err, count):
    """sqrt(E / count): the relative error of E halves under the root; the division (u, halved) and the root (u) add 3/2 u.
    -> (rmse from a 60-digit Decimal quotient and root, their 1e-50 counted in, bound)"""
    if count == 0:
        return Fraction(0), Fraction(0)
    decimal.getcontext().prec = 60
    q = err.values[0] / count
    root = Fraction((decimal.Decimal(q.numerator) / decimal.Decimal(q.denominator)).sqrt())
    if root == 0:
        return Fraction(0), Fraction(0)
    rel = err.first_order(0) / err.values[0] / 2 + U * 3 / 2 + Fraction(1, 10 ** 50)
    return root, 2 * root * rel


def info_entries(ex, count):
    """the 6 x 6 matrix m3d_information_matrix assembles from the moments -> {(a, b): (exact, bound)}, upper triangle"""
    neg = lambda k: (-ex.values[k], ex.bound(k))
    pos = lambda k: (ex.values[k], ex.bound(k))
    c = (Fraction(count), Fraction(0))
    z = (Fraction(0), Fraction(0))
    E = {(0, 0): derived_sum2(ex, 4, 5), (0, 1): neg(6), (0, 2): neg(7), (0, 3): z, (0, 4): neg(2), (0, 5): pos(1),
         (1, 1): derived_sum2(ex, 3, 5), (1, 2): neg(8), (1, 3): pos(2), (1, 4): z, (1, 5): neg(0),
         (2, 2): derived_sum2(ex, 3, 4), (2, 3): neg(1), (2, 4): pos(0), (2, 5): z,
         (3, 3): c, (3, 4): z, (3, 5): z, (4, 4): c, (4, 5): z, (5, 5): c}
    return E


# ---------------------------------------------------------------------------------------------- the kernels' order, in numpy
MUTANTS = ("drop_last_trip", "skip_65536", "skip_last_thread", "final_255_records", "final_nv_minus_1", "include_unmatched",
           "mean_over_n_src")
ICP_ONLY_MUTANTS = ("include_unmatched", "mean_over_n_src")


def _tree256(a):
    """tree_reduce_256 over axis 0 (256 leaves): off = 128 .. 1, a[t] += a[t + off] for t < off"""
    a = a.copy()
    off = 128
    while off > 0:
        a[:off] += a[off:2 * off]
        off >>= 1
    return a[0]


def emulate_sum(terms, mutant=None):
    """terms (n, NV) -> the NV sums as <<<256, 256>>> + kabsch_final_k<NV> add them: thread b * 256 + t adds the rows
    b * 256 + t + 65536 l serially, a tree over t, a tree over b"""
    terms = np.asarray(terms, dtype=np.float64)
    n, nv = terms.shape
    L = max(1, -(-n // STRIDE))
    pad = np.zeros((L * STRIDE, nv))
    pad[:n] = terms
    if mutant == "skip_65536" and n > 65536:
        pad[65536] = 0.0
    if mutant == "skip_last_thread" and n > 0:
        b = min(255, (n - 1) // 256)
        t = 255 if n >= (b + 1) * 256 else (n - 1) % 256
        pad[b * 256 + t::STRIDE] = 0.0
    trips = pad.reshape(L, STRIDE, nv)
    if mutant == "drop_last_trip" and L > 1:
        trips = trips[:L - 1]
    acc = np.zeros((STRIDE, nv))
    with np.errstate(invalid="ignore", over="ignore"):
        for chunk in trips:
            acc = acc + chunk
        rec = _tree256(acc.reshape(256, 256, nv).transpose(1, 0, 2))   # (thread, block, nv) -> records (block, nv)
        if mutant == "final_255_records":
            rec = rec.copy()
            rec[255] = 0.0
        out = _tree256(rec)
    if mutant == "final_nv_minus_1":
        out = out.copy()
        out[nv - 1] = 0.0
    return out


def _pair_terms(s, d, ms, md):
    with np.errstate(invalid="ignore", over="ignore"):
        sc, dc = s - ms, d - md
        cov = [dc[:, r] * sc[:, c] for r in range(3) for c in range(3)]
        var = [sc[:, c] * sc[:, c] for c in range(3)]
    return np.stack(cov + var, axis=1)


def emulate_kabsch(src, dst, mutant=None):
    src, dst = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(dst, dtype=np.float64).reshape(-1, 3)
    n = len(src)
    s0 = emulate_sum(np.hstack([src, dst]), mutant)
    inv = 1.0 / float(n)
    s1 = emulate_sum(_pair_terms(src, dst, s0[:3] * inv, s0[3:] * inv), mutant)
    return np.concatenate([s0, s1])


def emulate_icp(src, dst, max_dist, T, mutant=None, ref=None):
    """m3d_bench_icp_sums' 29 outputs in the kernels' order, from the reference's own correspondences (ref: an IcpExact of
    the same input, whose search is then not repeated)"""
    src, dst = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(dst, dtype=np.float64).reshape(-1, 3)
    n = len(src)
    moved = ref.moved if ref is not None else move(src, T)
    corr, d2 = (ref.corr, ref.d2) if ref is not None else brute_correspondences(moved, dst, max_dist)
    m = corr >= 0
    err = emulate_sum(np.stack([np.where(m, d2, 0.0), m.astype(np.float64)], axis=1), mutant)
    used = np.ones(n, dtype=bool) if mutant == "include_unmatched" else m
    j = np.where(m, corr, 0)                                   # (the mutant reads target 0 for an unmatched row)
    s = np.where(used[:, None], moved, 0.0)
    d = np.where(used[:, None], dst[j], 0.0)
    s0 = emulate_sum(np.hstack([s, d]), mutant)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / (float(n) if mutant == "mean_over_n_src" else err[1])
        ms, md = s0[:3] * inv, s0[3:] * inv
    t1 = np.where(used[:, None], _pair_terms(np.where(used[:, None], moved, 0.0), d, ms, md), 0.0)
    s1 = emulate_sum(t1, mutant)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        info = emulate_sum(np.stack([x, y, z, x * x, y * y, z * z, x * y, x * z, y * z], axis=1), mutant)
    return np.concatenate([err, s0, s1, info]), corr


# ---------------------------------------------------------------------------------------------- the input families
KABSCH_FAMILIES = ("integers", "probe_last", "ordinary", "offset", "cancellation", "nan")
KABSCH_EXACT_FAMILIES = ("integers",)
ICP_FAMILIES = ("integers", "probe_last", "ordinary", "offset", "cancellation", "nonfinite") + tuple("mask_" + m for m in MASKS)
ICP_EXACT_FAMILIES = ("integers",)
OFFSET = np.array([1e6, -2e6, 5e5])


def _pairs_zero_sum(n, rng):
    """n integer rows, |x| <= 2^10, in +/- pairs (rows 2k + o, 2k + 1 + o), the origin first when n is odd: every column sums
    to exactly 0 and row n - 1 is not zero"""
    half = rng.integers(-1024, 1025, size=(n // 2, 3)).astype(np.float64)
    half[np.all(half == 0, axis=1)] = 1.0
    out = np.zeros((n, 3))
    o = n % 2
    out[o::2], out[o + 1::2] = half, -half
    return out


def probe_positions(n):
    return sorted({p % n for p in PROBE_POSITIONS if p < n})


def _ordinary_pairs(n, seed):
    rng = np.random.default_rng(seed)
    src = rng.uniform(-1.0, 1.0, size=(n, 3))
    T = iu.truth_pose()
    dst = src @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.001, size=(n, 3))
    return np.ascontiguousarray(src), np.ascontiguousarray(dst)


def _big_positions(n):
    """(index of the 1e12 term, index of its negative): the former at or beyond 65536 where the size has such a row"""
    if n < 3:
        return None
    return (65536 + 7 if n > 65536 + 8 else n // 2), n - 1


def _cancelling(n, rng, scale=1e8, big=1e12):
    """rows 2k, 2k + 1 = +P_k + noise, -P_k + noise with |P_k| ~ scale; one row of +big at _big_positions, -big in row n - 1"""
    P = rng.uniform(0.5, 1.0, size=((n + 1) // 2, 3)) * rng.choice([-1.0, 1.0], size=((n + 1) // 2, 3)) * scale
    out = np.empty((n, 3))
    out[0::2], out[1::2] = P[:(n + 1) // 2], -P[:n // 2]
    out += rng.normal(0, 1.0, size=(n, 3))
    pos = _big_positions(n)
    if pos:
        out[pos[0]], out[pos[1]] = big * np.array([1.0, -1.0, 1.0]), -big * np.array([1.0, -1.0, 1.0])
    return out


def kabsch_probe(n, p):
    src, dst = np.zeros((n, 3)), np.zeros((n, 3))
    src[p], dst[p] = (3.0, -5.0, 7.0), (-2.0, 11.0, 13.0)
    return src, dst


@functools.lru_cache(maxsize=None)
def kabsch_input(family, n):
    """-> (src, dst), n x 3 each"""
    if family == "integers":
        rng = np.random.default_rng([1, n])
        return _pairs_zero_sum(n, rng), _pairs_zero_sum(n, rng)
    if family == "probe_last":
        return kabsch_probe(n, n - 1)
    if family == "ordinary":
        return _ordinary_pairs(n, [2, n])
    if family == "offset":
        s, d = _ordinary_pairs(n, [2, n])
        return s + OFFSET, d + OFFSET
    if family == "cancellation":
        rng = np.random.default_rng([3, n])
        return _cancelling(n, rng), _cancelling(n, rng)
    if family == "nan":
        s, d = _ordinary_pairs(n, [4, n])
        s = s.copy()
        s[min(65536, n - 1)] = np.nan
        return s, d
    raise KeyError(family)


@functools.lru_cache(maxsize=None)
def kabsch_exact(family, n):
    return exact_kabsch(*kabsch_input(family, n))


# the exact-integer ICP target: the lattice (4 i + 2, 4 j + 2, 4 k + 2), i, j, k in [-3, 3): 216 points, symmetric about the origin
def _lattice():
    a = 4.0 * np.arange(-3, 3) + 2.0
    return np.ascontiguousarray(np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3))


def icp_probe(n, p):
    """every moving point at the origin on the target point 0 = the origin, but row p one step beside target 1"""
    dst = np.array([[0.0, 0.0, 0.0], [8.0, -16.0, 32.0]])
    src = np.zeros((n, 3))
    src[p] = dst[1] + (1.0, 0.0, 0.0)
    return dict(src=src, dst=dst, max_dist=1.5, T=np.eye(4))


def _icp_ordinary(n, seed):
    p = iu.icp_pair(256, seed=seed)
    rng = np.random.default_rng([5, n, seed])
    src = p["src"][np.arange(n) % 256] + rng.normal(0, 0.002, size=(n, 3))
    return dict(src=np.ascontiguousarray(src), dst=p["dst"], max_dist=0.05, T=iu.offset_pose(p["T"], 0.5, (0.004, -0.002, 0.003)))


def mask_rows(n, mask):
    i = np.arange(n)
    return {"all": i >= 0, "none": i < 0, "ge65536": i >= 65536, "last": i == n - 1, "every_second": i % 2 == 0}[mask]


@functools.lru_cache(maxsize=None)
def icp_input(family, n):
    """-> dict(src (n x 3), dst (<= 1024 x 3), max_dist, T)"""
    if family == "integers":
        L = _lattice()
        if n == 1:
            return dict(src=L[:1] + (1.0, 0.0, 0.0), dst=L, max_dist=1.5, T=np.eye(4))
        k = np.arange(n // 2) % len(L)
        half = L[k] + np.where((np.arange(n // 2) // len(L)) % 2 == 0, 1.0, -1.0)[:, None] * np.array([1.0, 0.0, 0.0])
        src = np.zeros((n, 3))            # (odd n: row 0 is the origin, which no lattice point is near)
        o = n % 2
        src[o::2], src[o + 1::2] = half, -half
        return dict(src=src, dst=L, max_dist=1.5, T=np.eye(4))
    if family == "probe_last":
        return icp_probe(n, n - 1)
    if family == "ordinary":
        return _icp_ordinary(n, 31)
    if family == "offset":
        c = _icp_ordinary(n, 32)
        return dict(src=move(c["src"], c["T"]) + OFFSET, dst=c["dst"] + OFFSET, max_dist=c["max_dist"], T=np.eye(4))
    if family == "cancellation":
        # the target: 64 integer points of magnitude 1e8, their negatives, and +/- (1e12, -1e12, 1e12); the moving rows 2k,
        # 2k + 1 lie within a few units of +P, -P in turn, the two big ones at _big_positions.  The radius is a twentieth of
        # the extent (every point has its correspondence either way): the target grid stays a few hundred thousand cells
        rng = np.random.default_rng([6, n])
        P = np.round(rng.uniform(0.5, 1.0, size=(64, 3)) * rng.choice([-1.0, 1.0], size=(64, 3)) * 1e8)
        B = 1e12 * np.array([[1.0, -1.0, 1.0]])
        dst = np.concatenate([P, -P, B, -B])
        i = np.arange(n)
        src = dst[(i // 2) % 64 + 64 * (i % 2)] + rng.normal(0, 1.0, size=(n, 3))
        pos = _big_positions(n)
        if pos:
            src[pos[0]], src[pos[1]] = dst[128] + (1.0, 2.0, -1.0), dst[129] + (-2.0, 1.0, 1.0)
        return dict(src=np.ascontiguousarray(src), dst=np.ascontiguousarray(dst), max_dist=1e11, T=np.eye(4))
    if family == "nonfinite":
        c = _icp_ordinary(n, 33)
        src, dst = c["src"].copy(), np.vstack([c["dst"], [[np.inf, 0.0, 0.0]]])
        src[nonfinite_row(n)] = np.nan
        return dict(src=src, dst=dst, max_dist=c["max_dist"], T=c["T"])
    if family.startswith("mask_"):
        c = _icp_ordinary(n, 34)
        src = c["src"].copy()
        src[~mask_rows(n, family[5:])] += 100.0
        return dict(src=src, dst=c["dst"], max_dist=c["max_dist"], T=c["T"])
    raise KeyError(family)


def nonfinite_row(n):
    return min(65536, n - 1)


def nonfinite_clean(n):
    """the nonfinite family's input without its NaN moving point (moved out of reach instead) and without its Inf target"""
    c = icp_input("nonfinite", n)
    src = c["src"].copy()
    src[nonfinite_row(n)] = 100.0
    return dict(src=src, dst=c["dst"][:-1], max_dist=c["max_dist"], T=c["T"])


@functools.lru_cache(maxsize=None)
def icp_exact(family, n):
    c = icp_input(family, n)
    return IcpExact(c["src"], c["dst"], c["max_dist"], c["T"])


def same_bits(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))
