"""The writers' pool of the mask expansion (misc3d_amd/csrc/m3d_mask_pool.hpp), CPU only: a stand-alone program around the
header.  The list the pool writes is the plain bit loop's with nothing stored outside it -- with helpers and without, with a
second caller while the pool is busy (that one expands alone), under an affinity mask of two CPUs, and on a host whose sysfs
tells no topology; a count that disagrees is refused.  Built once more with the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR_DIR = os.path.join(ROOT, "misc3d_amd", "csrc")

PROGRAM = r"""
#include "m3d_mask_pool.hpp"

#include <cstdio>
#include <string>
#include <thread>
#include <vector>

using namespace m3d;

static const uint64_t kCanary = 0xDEADBEEFCAFEF00Dull;

struct Case {
    uint64_t n;
    std::vector<uint64_t> mask;
    std::vector<uint32_t> counts;
    std::vector<uint64_t> ref;
};
static Case make_case(uint64_t n, unsigned percent) {
    Case c;
    c.n = n;
    const uint32_t nb = (uint32_t)((n + 2047) / 2048);
    c.mask.assign((size_t)nb * kMaskTileWords + 1, 0);
    c.counts.assign(nb + 1, 0);
    uint64_t s = 0x9E3779B97F4A7C15ull ^ n;
    for (uint64_t i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        if ((s >> 40) % 100 < percent) {
            c.mask[i / 64] |= 1ull << (i % 64);
            ++c.counts[i / 2048];
            c.ref.push_back(i);
        }
    }
    return c;
}
// one expansion through the pool; 0: the list is the bit loop's and every word around it is still the canary
static int expand_once(const Case& c, uint32_t writers, unsigned offset) {
    std::vector<uint64_t> buf(c.ref.size() + 32, kCanary);
    uint64_t* dst = buf.data() + 8 + offset;
    MaskPool::get().arm(writers, 200);
    if (!MaskPool::get().expand(c.mask.data(), c.n, c.counts.data(), dst, writers)) return 1;
    for (size_t i = 0; i < buf.size(); ++i) {
        const uint64_t* p = buf.data() + i;
        const bool inside = p >= dst && p < dst + c.ref.size();
        if (*p != (inside ? c.ref[(size_t)(p - dst)] : kCanary)) return 1;
    }
    return 0;
}

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "all";
    int failures = 0;
    const std::vector<Case> cases = {make_case(1, 100), make_case(2049, 50), make_case(70001, 50), make_case(300001, 97),
                                     make_case(70001, 0)};
    if (what == "no_topology") MaskPool::get().sysfs_cpu = "/nonexistent";
    if (what == "two_cpus") {   // the first two CPUs of the mask this process has
        cpu_set_t have, two;
        CPU_ZERO(&have);
        CPU_ZERO(&two);
        if (sched_getaffinity(0, sizeof(have), &have) == 0)
            for (int c = 0, k = 0; c < CPU_SETSIZE && k < 2; ++c)
                if (CPU_ISSET(c, &have)) {
                    CPU_SET(c, &two);
                    ++k;
                }
        if (CPU_COUNT(&two) == 0 || sched_setaffinity(0, sizeof(two), &two) != 0) {
            std::printf("FAIL two_cpus: no affinity mask to set\n");
            return 1;
        }
        if (MaskPool::writer_cap(1) > (uint32_t)CPU_COUNT(&two)) {
            std::printf("FAIL two_cpus: more writers than CPUs in the mask\n");
            ++failures;
        }
    }
    if (what == "busy") {
        // two callers at once, many times: one of them finds the pool busy and expands alone
        for (int t = 0; t < 2; ++t) failures += expand_once(cases[2], 4, 0);
        std::vector<int> bad(2, 0);
        std::vector<std::thread> th;
        for (int t = 0; t < 2; ++t)
            th.emplace_back([&, t] {
                for (int r = 0; r < 200; ++r) bad[t] += expand_once(cases[1 + t], 4, (unsigned)t);
            });
        for (auto& t : th) t.join();
        failures += bad[0] + bad[1];
    } else if (what == "disagree") {
        Case c = cases[2];
        c.counts[3] += 1;
        std::vector<uint64_t> buf(c.ref.size() + 33, kCanary);
        MaskPool::get().arm(4, 200);
        if (MaskPool::get().expand(c.mask.data(), c.n, c.counts.data(), buf.data() + 8, 4)) ++failures;
        for (size_t i = 0; i < 8; ++i) failures += buf[i] != kCanary;
        for (size_t i = 8 + c.ref.size() + 1; i < buf.size(); ++i) failures += buf[i] != kCanary;
        failures += expand_once(cases[2], 4, 0);   // and the pool is usable afterwards
    } else {
        const uint32_t cap = what == "two_cpus" ? MaskPool::writer_cap(1) : 8u;
        for (int round = 0; round < 3; ++round)   // (jobs of different span counts behind each other)
            for (const Case& c : cases)
                for (uint32_t writers : {1u, 2u, 3u, cap})
                    for (unsigned offset : {0u, 3u}) failures += expand_once(c, writers, offset);
    }
    std::printf("%s: %d failures\n", what.c_str(), failures);
    return failures ? 1 : 0;
}
"""


def _build(d, extra):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    src = d / "pool.cpp"
    src.write_text(PROGRAM)
    exe = d / "pool"
    subprocess.run([cxx, "-O2", "-g", "-std=c++17", "-pthread", *extra, "-I", HDR_DIR, str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("mask_pool"), [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("mask_pool_san"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, what):
    r = subprocess.run([exe, what], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert f"{what}: 0 failures" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("what", ["lists", "busy", "disagree", "two_cpus", "no_topology"])
def test_pool(program, what):
    _run(program, what)


@pytest.mark.parametrize("what", ["lists", "busy", "two_cpus"])
def test_pool_under_address_and_undefined_sanitizers(sanitized, what):
    _run(sanitized, what)
