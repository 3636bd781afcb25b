"""The registration sums on the MI355X -- umeyama_sums_k with both of its pair sources (the record keys "kabsch_sums_k" and
"icp_sums_k"), icp_err_k, info_sums_k and kabsch_final_k, through the
test hooks m3d_bench_kabsch_sums and m3d_bench_icp_sums -- against the exact reference of tests/reg_sums_ref_util.py at every
seam of their reduction (the workgroup edge 255 / 256 / 257, the grid-stride edge 65535 / 65536 / 65537, three trips at
131073): bit for bit on the exact-integer and probe inputs, within the bound derived from the summation shape (factor 2 over
first order; the module's docstring) on all others, no tolerance a bare constant.  The public calls are tied to the hooks:
m3d_kabsch is the host assembly of the hook's sums bit for bit, m3d_information_matrix lies entry by entry within the moments'
bounds, one ICP iteration reports the exact fitness and an rmse within its bound.  tests/test_reg_sums.py shows on the CPU that
these checks notice a dropped trip, a skipped index, a record or value too few in the final tree, unmatched rows summed, and
means over the wrong count.  Every line "RATIO kernel n family |got - exact| / bound" is for the record, not a criterion."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import reg_sums_ref_util as ru
from test_reg_sums import icp_probe_expected

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device")
    return capi


@pytest.fixture(scope="module")
def assemble(tmp_path_factory):
    """m3d_reg_fp.hpp umeyama_from_sums on the host: (18 sums, n, scaling) -> T (4 x 4)"""
    exe = str(tmp_path_factory.mktemp("kabsch_assemble") / "test_kabsch_assemble")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "test_kabsch_assemble.cpp"),
                    "-o", exe], check=True)

    def run(sums, n, scaling=False):
        words = " ".join("%016x" % w for w in np.asarray(sums, dtype=np.float64).view(np.uint64).tolist())
        r = subprocess.run([exe], input="%d %d %s\n" % (n, int(scaling), words), capture_output=True, text=True, timeout=60,
                           check=True)
        return np.array([int(w, 16) for w in r.stdout.split()], dtype=np.uint64).view(np.float64).reshape(4, 4)

    return run


def _icp_hook(dev, c):
    return dev.icp_sums(c["src"], c["dst"], c["max_dist"], c["T"])


def _record(kernel, n, family, ratio):
    print("RATIO %s %d %s %.4g" % (kernel, n, family, ratio))


# ---------------------------------------------------------------------------------------------- m3d_bench_kabsch_sums
@pytest.mark.parametrize("n", ru.KABSCH_SIZES)
@pytest.mark.parametrize("family", ru.KABSCH_FAMILIES)
def test_kabsch_sums_against_the_exact_reference(dev, family, n):
    src, dst = ru.kabsch_input(family, n)
    ex = ru.kabsch_exact(family, n)
    got = dev.kabsch_sums(src, dst)
    assert ru.same_bits(got, dev.kabsch_sums(src, dst))            # two calls, identical bits
    ratios = ex.ratios(got)
    _record("kabsch_sums_k", n, family, max(ratios))
    if family in ru.KABSCH_EXACT_FAMILIES:
        assert ru.same_bits(got, ex.rounded()), (got, ex.rounded())
    if family == "nan":                                            # exactly the sums the NaN row enters are NaN
        assert np.array_equal(np.isnan(got), np.array(ex.nan))
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("n", ru.KABSCH_SIZES)
def test_kabsch_position_probes(dev, n):
    for p in ru.probe_positions(n):
        src, dst = ru.kabsch_probe(n, p)
        got = dev.kabsch_sums(src, dst)
        assert ru.same_bits(got[:6], np.concatenate([src[p], dst[p]])), (n, p, got)


@pytest.mark.parametrize("n", ru.KABSCH_SIZES)
def test_kabsch_is_the_host_assembly_of_the_hooks_sums(dev, assemble, n):
    for family in ("integers", "ordinary", "offset", "cancellation"):
        src, dst = ru.kabsch_input(family, n)
        sums = dev.kabsch_sums(src, dst)
        for scaling in (False, True):
            assert ru.same_bits(dev.kabsch(src, dst, scaling=scaling), assemble(sums, n, scaling)), (family, n, scaling)


# ---------------------------------------------------------------------------------------------- m3d_bench_icp_sums
@pytest.mark.parametrize("n", ru.ICP_SIZES)
@pytest.mark.parametrize("family", ru.ICP_FAMILIES)
def test_icp_sums_against_the_exact_reference(dev, family, n):
    c = ru.icp_input(family, n)
    ex = ru.icp_exact(family, n)
    got, corr = _icp_hook(dev, c)
    assert np.array_equal(corr, ex.corr)                           # the correspondence set first: the reference's own
    got2, corr2 = _icp_hook(dev, c)
    assert ru.same_bits(got, got2) and np.array_equal(corr, corr2)
    assert not np.isnan(got).any()                                 # (no 1 / count of an empty set reaches the output)
    assert got[1] == ex.count
    ratios = ex.ratios(got)
    for kernel, r in ratios.items():
        _record(kernel, n, family, r)
    if family in ru.ICP_EXACT_FAMILIES:
        assert ru.same_bits(got, ex.rounded()), (got, ex.rounded())
        assert got[0] == got[1] == ex.count                        # every d2 is exactly 1
    if ex.count == 0:
        assert not got.any()
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("n", ru.ICP_SIZES)
def test_icp_position_probes(dev, n):
    for p in ru.probe_positions(n):
        c = ru.icp_probe(n, p)
        got, corr = _icp_hook(dev, c)
        e, raw, mom = icp_probe_expected(c, p)
        assert np.array_equal(corr, (np.arange(n) == p).astype(np.int64)), (n, p)
        assert ru.same_bits(got[0:2], e) and ru.same_bits(got[2:8], raw) and ru.same_bits(got[20:29], mom), (n, p, got)


@pytest.mark.parametrize("n", ru.ICP_SIZES)
def test_nonfinite_points_are_nobodys_correspondence(dev, n):
    """a NaN moving point and an Inf target point change nothing: the sums are, bit for bit, those of the cloud whose point
    is out of reach instead and whose target ends one row earlier"""
    dirty, clean = ru.icp_input("nonfinite", n), ru.nonfinite_clean(n)
    got, corr = _icp_hook(dev, dirty)
    want, corr_clean = _icp_hook(dev, clean)
    assert corr[ru.nonfinite_row(n)] == -1 and not np.any(corr == len(dirty["dst"]) - 1)
    assert np.array_equal(corr, corr_clean) and ru.same_bits(got, want)


# ---------------------------------------------------------------------------------------------- the public calls on the same inputs
@pytest.mark.parametrize("n", ru.ICP_SIZES)
@pytest.mark.parametrize("family", ("integers", "ordinary", "offset", "cancellation", "mask_every_second", "mask_none"))
def test_information_matrix_entry_by_entry(dev, family, n):
    c = ru.icp_input(family, n)
    ex = ru.icp_exact(family, n)
    info, count = dev.information_matrix(c["src"], c["dst"], c["max_dist"], c["T"])
    assert count == ex.count and info[3, 3] == info[4, 4] == info[5, 5] == ex.count
    assert ru.same_bits(info, info.T)
    worst = 0.0
    for (a, b), (value, bound) in ru.info_entries(ex.info, ex.count).items():
        err = abs(Fraction(float(info[a, b])) - value)
        assert err <= bound, (a, b, float(info[a, b]), float(value), float(bound))
        worst = max(worst, float(err / bound) if bound else 0.0)
    _record("m3d_information_matrix", n, family, worst)
    if family in ru.ICP_EXACT_FAMILIES:
        hook, _ = _icp_hook(dev, c)
        m = hook[20:29]
        assert ru.same_bits([info[0, 0], info[1, 1], info[2, 2], info[0, 1], info[2, 4]], [m[4] + m[5], m[3] + m[5], m[3] + m[4], -m[6], m[0]])


@pytest.mark.parametrize("n", (257, 65537))
def test_one_icp_iteration_reports_what_the_sums_imply(dev, assemble, n):
    """registration_icp(max_iteration = 1): the update is the host assembly of the hook's sums under the initial pose, the
    moving cloud goes through both transformations in turn, and the result is the evaluation at that second position"""
    c = ru.icp_input("ordinary", n)
    first = ru.icp_exact("ordinary", n)
    out, corr0 = _icp_hook(dev, c)
    assert np.array_equal(corr0, first.corr) and out[1] == first.count
    update = assemble(out[2:20], first.count, False)
    moved = ru.move(first.moved, update)
    ex = ru.IcpExact(moved, c["dst"], c["max_dist"], np.eye(4))
    _, st, corr = dev.registration_icp(c["src"], c["dst"], c["max_dist"], c["T"], max_iteration=1, want_correspondences=True)
    assert st["iterations"] == 1
    assert np.array_equal(corr, ex.corr) and st["correspondences"] == ex.count
    assert st["fitness"] == ex.count / n
    rmse, bound = ru.derived_rmse(ex.err, ex.count)
    err = abs(Fraction(st["inlier_rmse"]) - rmse)
    _record("rmse", n, "ordinary", float(err / bound))
    assert err <= bound, (st["inlier_rmse"], float(rmse), float(bound))
