"""The planes' reference-histogram bound on the host (no GPU): tests/cpp/test_ref_hist_bound.cpp runs ref_pair_ub
(misc3d_amd/csrc/m3d_bound_fp.hpp: the code plane_bound_k runs on the device, compiled by g++) against exact counts."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BUILD = os.path.join(CPP, "_build")


def _build(name, *defs):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *defs, os.path.join(CPP, "test_ref_hist_bound.cpp"), "-o", exe],
                   check=True, capture_output=True)
    return exe


def test_reference_histogram_bound_holds_on_the_host():
    """Random tiles (flat, clutter, mixed, NaN-padded) up to 300 scene sizes from the origin; hypotheses 0 .. 5 degrees off the
    reference, antiparallel, at the cosine limit, with interval ends exactly on bin edges and beyond the span: the bound is never
    below the exact count -- at the bin count the library is built with and at the two others that were measured.  The second
    build drops the margins and the outward bins (M3D_BOUND_NO_SLACK): it must report violations, i.e. the pairs probe them."""
    for bins in (64, 32, 128):
        r = subprocess.run([_build(f"test_ref_hist_bound_{bins}", f"-DM3D_REF_BINS={bins}"), "6000"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "all checks passed" in r.stdout and "violations 0" in r.stdout, r.stdout + r.stderr
    m = subprocess.run([_build("test_ref_hist_bound_no_slack", "-DM3D_BOUND_NO_SLACK"), "6000"], capture_output=True, text=True, timeout=300)
    assert m.returncode != 0 and "all checks passed" not in m.stdout
    assert int(re.search(r"violations (\d+)", m.stdout).group(1)) > 1000, m.stdout
