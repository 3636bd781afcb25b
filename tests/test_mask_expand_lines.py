"""The span form of the inlier-mask expansion (misc3d_amd/csrc/m3d_mask_expand.hpp: mask_split_lines, mask_expand_span), CPU
only.  A stand-alone program around the header, built with the system compiler, writes every span of every case ALONE into a
destination that holds a canary word in every entry -- in front of the list, behind it and in every other span -- and compares
entry by entry with a plain bit loop: the span's entries are the list's, every other word is still the canary.  The portable
loop and the AVX-512 path go through the same cases; the same program is built once more with the address and
undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR_DIR = os.path.join(ROOT, "misc3d_amd", "csrc")

PROGRAM = r"""
#include "m3d_mask_expand.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace m3d;

static const uint64_t kCanary = 0xDEADBEEFCAFEF00Dull;
static const uint64_t kFront = 24;   // canary entries in front of the list and behind it (three lines each)

static const uint64_t kSizes[] = {0, 1, 63, 64, 65, 2047, 2048, 2049, 70001};
static const char* kMasks[] = {"empty", "full", "first", "last", "alternating", "half", "one_full_tile"};

static std::vector<uint8_t> flags_for(const std::string& kind, uint64_t n) {
    std::vector<uint8_t> f(n, 0);
    uint64_t s = 0x9E3779B97F4A7C15ull ^ n;
    for (uint64_t i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        if (kind == "full") f[i] = 1;
        else if (kind == "first") f[i] = i == 0;
        else if (kind == "last") f[i] = i == n - 1;
        else if (kind == "alternating") f[i] = i & 1;
        else if (kind == "half") f[i] = (s >> 40) & 1;
        else if (kind == "one_full_tile") f[i] = i < 2048;
    }
    return f;
}

struct Case {
    uint64_t n = 0;
    uint32_t nb = 0;
    std::vector<uint64_t> mask;     // whole tiles, as the device writes them
    std::vector<uint32_t> counts;
    std::vector<uint64_t> ref;      // the plain bit loop
};
static Case make_case(const std::vector<uint8_t>& f) {
    Case c;
    c.n = f.size();
    c.nb = (uint32_t)((c.n + 2047) / 2048);
    c.mask.assign((size_t)c.nb * kMaskTileWords + 1, 0);   // (+1: never an empty vector's null pointer)
    c.counts.assign(c.nb + 1, 0);
    for (uint64_t i = 0; i < c.n; ++i)
        if (f[i]) {
            c.mask[i / 64] |= 1ull << (i % 64);
            ++c.counts[i / 2048];
            c.ref.push_back(i);
        }
    return c;
}

// every span of `parts` written alone at `offset` entries past a 64-byte line; 0: as it must be
static int check(const Case& c, const std::vector<uint32_t>& counts, uint32_t parts, unsigned offset, int path, bool expect_ok,
                 const char* what) {
    std::vector<uint64_t> prefix(c.nb + 1);
    const uint64_t total = mask_tile_prefix(counts.data(), c.nb, prefix.data());
    const size_t words = kFront + 8 + total + kFront;
    uint64_t* raw = static_cast<uint64_t*>(std::aligned_alloc(64, (words * 8 + 63) / 64 * 64));
    uint64_t* dst = raw + kFront + offset;
    std::vector<uint64_t> cuts(parts + 1);
    mask_split_lines(total, parts, dst, cuts.data());
    int bad = 0;
    if (cuts[0] != 0 || cuts[parts] != total) bad = 1;
    for (uint32_t k = 0; k < parts && !bad; ++k) {
        if (cuts[k] > cuts[k + 1]) bad = 1;
        if (k && cuts[k] != total && cuts[k] != 0 && ((uintptr_t)(dst + cuts[k]) & 63u)) bad = 1;   // a span begins on a line
    }
    bool all_ok = true;
    for (uint32_t k = 0; k < parts && !bad; ++k) {
        for (size_t i = 0; i < words; ++i) raw[i] = kCanary;
        const bool ok = mask_expand_span(c.mask.data(), c.n, prefix.data(), c.nb, cuts[k], cuts[k + 1], dst, path);
        all_ok = all_ok && ok;
        for (size_t i = 0; i < words && !bad; ++i) {
            const uint64_t* p = raw + i;
            const bool inside = p >= dst + cuts[k] && p < dst + cuts[k + 1];
            if (!inside && *p != kCanary) bad = 2;                                                  // a store left its span
            if (inside && ok && expect_ok && *p != c.ref[(size_t)(p - dst)]) bad = 3;               // a wrong entry
        }
    }
    if (!bad && all_ok != expect_ok) bad = 4;
    if (bad)
        std::printf("FAIL %s: n %llu parts %u offset %u path %d: %s\n", what, (unsigned long long)c.n, parts, offset, path,
                    bad == 1 ? "cuts" : bad == 2 ? "a canary was overwritten" : bad == 3 ? "a wrong entry" : "return value");
    std::free(raw);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "all";
    const int paths = mask_have_avx512() ? 2 : 1;   // 0: the portable loop; 1: AVX-512
    int failures = 0;
    long cases = 0;
    if (what == "all" || what == "matrix") {
        for (uint64_t n : kSizes)
            for (const char* kind : kMasks) {
                const Case c = make_case(flags_for(kind, n));
                const uint32_t part_list[] = {1, 2, 3, 8, 32, c.nb + 5};
                for (uint32_t parts : part_list)
                    for (unsigned offset = 0; offset < 8; ++offset)
                        for (int f = 0; f < paths; ++f, ++cases)
                            failures += check(c, c.counts, parts, offset, f, true, kind);
            }
    }
    if (what == "all" || what == "disagree") {
        // one bit more, or one fewer, in a tile than its count says -- in the first, a middle and the last tile
        const Case c = make_case(flags_for("half", 70001));
        for (uint32_t t : {0u, c.nb / 2, c.nb - 1})
            for (int d : {-1, 1}) {
                std::vector<uint32_t> counts = c.counts;
                counts[t] = (uint32_t)((int)counts[t] + d);
                for (uint32_t parts : {1u, 3u, 8u, 32u})
                    for (unsigned offset : {0u, 5u})
                        for (int f = 0; f < paths; ++f, ++cases)
                            failures += check(c, counts, parts, offset, f, false, "disagree");
            }
    }
    if (what == "all" || what == "disagree") {
        // a stray bit in a tile whose count is 0: right behind the full tile, in the middle, in the last tile; and behind a list of one
        for (const char* kind : {"one_full_tile", "first"}) {
            const Case c = make_case(flags_for(kind, 70001));
            for (uint32_t t : {1u, c.nb / 2, c.nb - 1}) {
                Case stray = c;
                stray.mask[(size_t)t * kMaskTileWords + 3] |= 1ull << 17;
                for (uint32_t parts : {1u, 3u, 8u, 32u})
                    for (unsigned offset : {0u, 5u})
                        for (int f = 0; f < paths; ++f, ++cases)
                            failures += check(stray, c.counts, parts, offset, f, false, "stray bit");
            }
        }
    }
    if (what == "all" || what == "threads") {
        // all spans at once, side by side on one destination, through the entry point the tests share with the library's pool
        for (uint64_t n : {2049ull, 70001ull})
            for (const char* kind : {"half", "full", "one_full_tile"}) {
                const Case c = make_case(flags_for(kind, n));
                for (uint32_t writers : {1u, 3u, 8u})
                    for (int f = 0; f < paths; ++f, ++cases) {
                        std::vector<uint64_t> buf(c.ref.size() + 16, kCanary);
                        const bool ok = mask_expand_spans_threads(c.mask.data(), c.n, c.counts.data(), buf.data() + 8, writers, f);
                        bool same = ok;
                        for (size_t i = 0; i < buf.size(); ++i) {
                            const bool inside = i >= 8 && i < 8 + c.ref.size();
                            same = same && buf[i] == (inside ? c.ref[i - 8] : kCanary);
                        }
                        if (!same) {
                            std::printf("FAIL threads %s: n %llu writers %u path %d\n", kind, (unsigned long long)n, writers, f);
                            ++failures;
                        }
                    }
            }
    }
    std::printf("%s: %ld cases, %d failures, avx512 %d\n", what.c_str(), cases, failures, (int)mask_have_avx512());
    return failures ? 1 : 0;
}
"""


def _compiler():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    return cxx


def _build(d, extra):
    src = d / "spans.cpp"
    src.write_text(PROGRAM)
    exe = d / "spans"
    subprocess.run([_compiler(), "-O2", "-g", "-std=c++17", "-pthread", *extra, "-I", HDR_DIR, str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("mask_spans"), [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("mask_spans_san"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, what):
    r = subprocess.run([exe, what], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert f"{what}:" in r.stdout and " 0 failures" in r.stdout, r.stdout[-2000:]


def test_every_span_alone_matches_the_bit_loop_and_keeps_the_canaries(program):
    """9 point counts x 7 masks x 8 offsets against a line x {1, 2, 3, 8, 32, tiles + 5} spans x both paths"""
    _run(program, "matrix")


def test_a_count_that_disagrees_is_refused_with_no_canary_touched(program):
    _run(program, "disagree")


def test_spans_side_by_side(program):
    _run(program, "threads")


def test_all_cases_under_address_and_undefined_sanitizers(sanitized):
    _run(sanitized, "all")
