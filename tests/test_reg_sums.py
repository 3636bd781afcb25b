"""The registration sums' reference, checked without a device (tests/reg_sums_ref_util.py): a numpy emulation of the kernels'
summation order stays inside the derived bound on every input family and size of tests/test_gpu_reg_sums.py and equals the exact
reference on the exact-integer families; every mutation of that order the GPU tests are meant to notice fails on at least one
family at one seam size; the exact reference agrees with math.fsum and with the oracle's serial sums."""
import math
from fractions import Fraction

import numpy as np
import pytest

import reg_sums_ref_util as ru


def _kabsch_violations(family, n, mutant=None):
    """what test_gpu_reg_sums.py would hold against the kernels, held against the emulation -> list of failures"""
    src, dst = ru.kabsch_input(family, n)
    got = ru.emulate_kabsch(src, dst, mutant)
    ex = ru.kabsch_exact(family, n)
    bad = []
    if family in ru.KABSCH_EXACT_FAMILIES and not ru.same_bits(got, ex.rounded()):
        bad.append("bits")
    if max(ex.ratios(got)) > 1.0:
        bad.append("bound")
    return bad


def _icp_violations(family, n, mutant=None):
    c = ru.icp_input(family, n)
    ex = ru.icp_exact(family, n)
    got, corr = ru.emulate_icp(c["src"], c["dst"], c["max_dist"], c["T"], mutant, ex)
    bad = []
    assert np.array_equal(corr, ex.corr)
    if family in ru.ICP_EXACT_FAMILIES and not ru.same_bits(got, ex.rounded()):
        bad.append("bits")
    if max(ex.ratios(got).values()) > 1.0:
        bad.append("bound")
    return bad


def _kabsch_probe_violations(n, p, mutant=None):
    src, dst = ru.kabsch_probe(n, p)
    got = ru.emulate_kabsch(src, dst, mutant)
    return [] if ru.same_bits(got[:6], np.concatenate([src[p], dst[p]])) else ["probe"]


def icp_probe_expected(c, p):
    """(error, count), the six raw sums and the nine moments of the probe input: exactly row p's values"""
    x, y, z = c["dst"][1]
    return np.array([1.0, float(len(c["src"]))]), np.concatenate([c["src"][p], c["dst"][1]]), np.array(
        [x, y, z, x * x, y * y, z * z, x * y, x * z, y * z])


def _icp_probe_violations(n, p, mutant=None):
    c = ru.icp_probe(n, p)
    got, _ = ru.emulate_icp(c["src"], c["dst"], c["max_dist"], c["T"], mutant)
    e, raw, mom = icp_probe_expected(c, p)
    ok = ru.same_bits(got[0:2], e) and ru.same_bits(got[2:8], raw) and ru.same_bits(got[20:29], mom)
    return [] if ok else ["probe"]


@pytest.mark.parametrize("n", ru.KABSCH_SIZES)
def test_emulated_kabsch_sums_hold_on_every_family(n):
    for family in ru.KABSCH_FAMILIES:
        assert _kabsch_violations(family, n) == [], (family, n)
    for p in ru.probe_positions(n):
        assert _kabsch_probe_violations(n, p) == [], (n, p)


@pytest.mark.parametrize("n", ru.ICP_SIZES)
def test_emulated_icp_sums_hold_on_every_family(n):
    for family in ru.ICP_FAMILIES:
        assert _icp_violations(family, n) == [], (family, n)
    for p in ru.probe_positions(n):
        assert _icp_probe_violations(n, p) == [], (n, p)


def test_families_are_what_they_claim():
    for n in ru.KABSCH_SIZES:
        for a in ru.kabsch_input("integers", n):
            assert np.all(a == np.round(a)) and np.abs(a).max() <= 1024 and np.all(a.sum(axis=0) == 0) and a[n - 1].any()
        ex = ru.kabsch_exact("offset", n)
        assert all(ex.abs[k] > 1e5 * n for k in range(6))                    # the pass-0 sums are large ...
        assert all(ex.abs[k] < 4 * n for k in range(6, 18))                  # ... the centred ones are not
        if n >= 255:
            s, _ = ru.kabsch_input("cancellation", n)
            ex = ru.kabsch_exact("cancellation", n)
            assert all(abs(ex.values[k]) < 1e-3 * ex.abs[k] for k in range(3))   # small true sums of large terms
            big = np.nonzero(np.abs(s[:, 0]) == 1e12)[0]
            assert len(big) == 2 and big[1] == n - 1 and (big[0] >= 65536 or n <= 65544)
    for n in ru.ICP_SIZES:
        ex = ru.icp_exact("integers", n)
        assert ex.count == n - (n % 2 if n > 1 else 0) and np.all(ex.d2[ex.matched] == 1.0)
        assert all(v == 0 for v in ex.sums.values[:6]) or n == 1
        for mask in ru.MASKS:
            assert np.array_equal(ru.icp_exact("mask_" + mask, n).matched, ru.mask_rows(n, mask)), (mask, n)
        ex = ru.icp_exact("nonfinite", n)
        dirty = ru.icp_input("nonfinite", n)
        assert ex.corr[ru.nonfinite_row(n)] == -1 and not np.any(ex.corr == len(dirty["dst"]) - 1)
        clean = ru.nonfinite_clean(n)
        assert np.array_equal(ex.corr, ru.brute_correspondences(ru.move(clean["src"], clean["T"]), clean["dst"], clean["max_dist"])[0])


# (hook, family or probe position, size) candidates per mutant, the cheap ones first; every mutant must fail one of them
_SEAMS = (257, 65537, 131073)


def _catch(mutant):
    for n in _SEAMS:
        for p in ru.probe_positions(n):
            if mutant not in ru.ICP_ONLY_MUTANTS and _kabsch_probe_violations(n, p, mutant):
                return "kabsch probe at %d, n = %d" % (p, n)
            if _icp_probe_violations(n, p, mutant):
                return "icp probe at %d, n = %d" % (p, n)
        for family in ru.ICP_FAMILIES:
            if _icp_violations(family, n, mutant):
                return "icp %s, n = %d" % (family, n)
        if mutant not in ru.ICP_ONLY_MUTANTS:
            for family in ru.KABSCH_FAMILIES:
                if _kabsch_violations(family, n, mutant):
                    return "kabsch %s, n = %d" % (family, n)
    return None


@pytest.mark.parametrize("mutant", ru.MUTANTS)
def test_every_mutant_of_the_order_is_caught(mutant):
    caught = _catch(mutant)
    print(mutant, "->", caught)
    assert caught is not None, mutant


def test_mutants_are_caught_in_both_hooks_and_by_the_integer_family():
    """beyond 'somewhere': the indexing mutants fail the bit comparison of the exact-integer family in BOTH hooks at the size
    that has their seam, and the two mean / mask mutants fail the masked ordinary cloud"""
    for mutant, n in (("drop_last_trip", 65537), ("skip_65536", 65537), ("skip_last_thread", 257), ("skip_last_thread", 65537),
                      ("final_255_records", 65536), ("final_nv_minus_1", 256)):
        assert "bits" in _kabsch_violations("integers", n, mutant), (mutant, n)
        assert "bits" in _icp_violations("integers", n, mutant), (mutant, n)
    for n in (257, 65537):
        assert _icp_violations("mask_every_second", n, "include_unmatched")
        assert _icp_violations("mask_every_second", n, "mean_over_n_src")
        assert _icp_violations("mask_none", n, "include_unmatched")


def test_exact_raw_sums_agree_with_fsum():
    for family in ("ordinary", "offset", "cancellation"):
        src, dst = ru.kabsch_input(family, 65537)
        ex = ru.kabsch_exact(family, 65537)
        want = [math.fsum(a[:, k]) for a in (src, dst) for k in range(3)]
        assert ru.same_bits(ex.rounded()[:6], want), family
        c, e = ru.icp_input(family, 65537), ru.icp_exact(family, 65537)
        assert e.err.rounded()[0] == math.fsum(e.d2[e.matched]) and e.count == len(e.d2[e.matched])
        assert ru.same_bits(e.info.rounded()[:3], [math.fsum(e.d[:, k]) for k in range(3)])
        assert ru.same_bits(e.sums.rounded()[:6], [math.fsum(a[:, k]) for a in (e.s, e.d) for k in range(3)])
        # the products, error-free: x y = p + e with p = fl(x y) and e from Dekker's split, both doubles
        x, y = e.d[:, 0], e.d[:, 1]
        assert e.info.rounded()[6] == math.fsum(_two_products(x, y)), family


def _two_products(x, y):
    p = x * y
    out = []
    for a, b, q in zip(x.tolist(), y.tolist(), p.tolist()):
        out += [q, float(Fraction(a) * Fraction(b) - Fraction(q))]   # (the remainder of one product is a double)
    return out


def test_exact_reference_against_the_oracle():
    """oracle.information_matrix adds the matched target points' moments serially (one rounding per product, m - 1 additions):
    its entries lie within ((m + 1) u sum |t|) (first order, doubled) of the exact moments.  oracle.umeyama's pose is held
    through its translation-free consequence: T maps the exact source mean on the exact target mean, up to the means' own
    serial error ((m + 2) u sum |x| / m per coordinate, carried through |R| <= 1) and the dozen roundings of the assembly."""
    import oracle
    c = ru.icp_input("ordinary", 4099)
    ex = ru.icp_exact("ordinary", 4099)
    info = oracle.information_matrix(c["src"], c["dst"], c["max_dist"], c["T"])
    m = ex.count
    assert m > 3000 and info[5, 5] == m and info[3, 3] == m and info[4, 4] == m
    serial = lambda k: 2 * (m + 1) * ru.U * ex.info.abs[k]
    for (a, b), k, sign in (((0, 1), 6, -1), ((0, 2), 7, -1), ((1, 2), 8, -1), ((0, 5), 1, 1), ((1, 3), 2, 1), ((2, 4), 0, 1),
                            ((0, 4), 2, -1), ((1, 5), 0, -1), ((2, 3), 1, -1)):
        assert abs(Fraction(float(info[a, b])) - sign * ex.info.values[k]) <= serial(k), (a, b)
        assert info[a, b] == info[b, a]
    for a, (k1, k2) in enumerate(((4, 5), (3, 5), (3, 4))):
        v = ex.info.values[k1] + ex.info.values[k2]
        assert abs(Fraction(float(info[a, a])) - v) <= serial(k1) + serial(k2) + 2 * ru.U * abs(v), a
    src, dst = ru.kabsch_input("ordinary", 4099)
    exk = ru.kabsch_exact("ordinary", 4099)
    T = oracle.umeyama(src, dst)
    n = len(src)
    ms, md = [exk.values[k] / n for k in range(3)], [exk.values[3 + k] / n for k in range(3)]
    for r in range(3):
        image = sum(Fraction(float(T[r, k])) * ms[k] for k in range(3)) + Fraction(float(T[r, 3]))
        slack = 2 * ru.U * ((n + 2) * (sum(exk.abs[k] for k in range(3)) + exk.abs[3 + r]) / n + 12 * (sum(abs(v) for v in ms) + abs(md[r])))
        assert abs(image - md[r]) <= slack, r


def test_hooks_check_their_arguments_and_fall_back_to_nothing(capi):
    """m3d_bench_kabsch_sums refuses what m3d_kabsch refuses, m3d_bench_icp_sums what m3d_registration_icp refuses; an empty
    cloud gives zeros and no correspondence (decided before a device is asked for); without a device both fail, loudly"""
    few, three = np.zeros((2, 3)), np.arange(9.0).reshape(3, 3)
    for call in (capi.kabsch_sums, capi.kabsch):
        with pytest.raises(capi.M3DError) as e:
            call(few, few)
        assert e.value.code == capi.ERR_TOO_FEW_POINTS
        with pytest.raises(capi.M3DError) as e:
            call(three, few)
        assert e.value.code == capi.ERR_SIZE_MISMATCH
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(capi.M3DError) as e:
            capi.icp_sums(three, three, bad, np.eye(4))
        assert e.value.code == capi.ERR_INVALID_ARG
    for src, dst in ((np.zeros((0, 3)), three), (three, np.zeros((0, 3)))):
        out, corr = capi.icp_sums(src, dst, 1.0, np.eye(4))
        assert out.shape == (29,) and not out.any() and np.array_equal(corr, np.full(len(src), -1))
    if capi.device_count() == 0:
        for call in (lambda: capi.kabsch_sums(three, three), lambda: capi.icp_sums(three, three, 1.0, np.eye(4))):
            with pytest.raises(capi.M3DError) as e:
                call()
            assert e.value.code == capi.ERR_DEVICE
