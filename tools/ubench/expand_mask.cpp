// expand_mask.cpp -- microbenchmark of the inlier-mask expansion (misc3d_amd/csrc/m3d_mask_expand.hpp, m3d_mask_pool.hpp): how
// long 8 and 12 writers take to write the index list of a mask, with three switches that separate what the library's expansion
// differs in from a plain host loop, and the whole-tile split of earlier builds beside the spans.  It links the library (the
// page-locked rows need m3d_host_alloc and a device); the portable loop and fewer writers are timed by no row here.
//
//   destination   pageable (a std::vector) | m3d_host_alloc (page-locked: hipHostMalloc, portable)
//   mask, counts  pageable, written by the host once | page-locked, written by a device kernel before EVERY repetition
//   writers       threads of this program that keep their stretch of the list | the library's MaskPool claiming spans
//   split         tiles (whole-tile ranges: the form before spans) | spans (of the list, beginning on 64-byte lines)
//
//   hipcc -O2 -std=c++17 -pthread --offload-arch=gfx950 -I misc3d_amd/csrc -I include tools/ubench/expand_mask.cpp \
//         -L misc3d_amd/lib -lmisc3d_amd -Wl,-rpath,'$ORIGIN/../../misc3d_amd/lib' -o tools/ubench/expand_mask
//   tools/ubench/expand_mask [MASK_FILE N]
// MASK_FILE: the mask as bytes, bit i of byte i / 8 = point i (np.packbits(flags, bitorder="little")), N points.  Without
// one: a C2-like mask of 1 000 000 points -- a plane holding every other 2048-point stretch, the rest clutter (~50 %).
// Without a device only the pageable rows run.  "read": the caller's sum over the list right after the expansion.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "m3d_mask_pool.hpp"
#include "misc3d_amd.h"

using namespace m3d;
using Clock = std::chrono::steady_clock;

__global__ void copy_words_k(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

enum { kTiles = 0, kSpans = 1 };

struct Job {
    const uint64_t* mask;
    const uint32_t* counts;
    uint64_t n;
    uint32_t nb;
    uint64_t* dst;
    const uint64_t* prefix;
    int form;
};

// writers of this program: writer k keeps part k of the list from repetition to repetition
struct OwnWriters {
    uint32_t writers;
    Job job{};
    std::vector<uint32_t> bounds;
    std::vector<uint64_t> cuts;
    std::atomic<int> go{0}, done{0};
    std::atomic<bool> quit{false};
    std::vector<std::thread> th;
    explicit OwnWriters(uint32_t w) : writers(w), bounds(w + 1), cuts(w + 1) {
        for (uint32_t k = 1; k < writers; ++k)
            th.emplace_back([this, k] {
                int seen = 0;
                for (;;) {
                    int g;
                    while ((g = go.load(std::memory_order_acquire)) == seen && !quit.load(std::memory_order_relaxed)) {
                    }
                    if (quit.load()) return;
                    seen = g;
                    part(k);
                    done.fetch_add(1, std::memory_order_release);
                }
            });
    }
    ~OwnWriters() {
        quit.store(true);
        for (auto& t : th) t.join();
    }
    void part(uint32_t k) {
        if (job.form == kTiles)
            mask_expand_range(job.mask, job.n, job.prefix, bounds[k], bounds[k + 1], job.dst);
        else
            mask_expand_span(job.mask, job.n, job.prefix, job.nb, cuts[k], cuts[k + 1], job.dst);
    }
    void expand(const Job& j) {
        job = j;
        if (j.form == kTiles) mask_split(j.prefix, j.nb, writers, bounds.data());
        else mask_split_lines(j.prefix[j.nb], writers, j.dst, cuts.data());
        done.store(0);
        go.fetch_add(1, std::memory_order_release);
        part(0);
        while (done.load(std::memory_order_acquire) != (int)writers - 1) {
        }
    }
};

static const char* form_name(int f) { return f == kTiles ? "tiles" : "spans"; }

int main(int argc, char** argv) {
    uint64_t n = 1000000;
    std::vector<uint64_t> mask;
    if (argc >= 3) {
        n = std::strtoull(argv[2], nullptr, 10);
        mask.assign((n + 64 * kMaskTileWords - 1) / (64 * kMaskTileWords) * kMaskTileWords, 0);
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 1;
        const size_t got = std::fread(mask.data(), 1, (n + 7) / 8, f);
        std::fclose(f);
        if (got != (n + 7) / 8) return 1;
    } else {
        mask.assign((n + 64 * kMaskTileWords - 1) / (64 * kMaskTileWords) * kMaskTileWords, 0);
        uint64_t s = 12345;
        for (uint64_t i = 0; i < n; ++i) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            const bool plane = ((i / 2048) & 1) == 0;
            if (plane ? (s >> 40) % 100 < 97 : (s >> 40) % 100 < 3) mask[i / 64] |= 1ull << (i % 64);
        }
    }
    const uint32_t nb = (uint32_t)(mask.size() / kMaskTileWords);
    const uint32_t n_words = (uint32_t)mask.size();
    std::vector<uint32_t> counts(nb);
    for (uint32_t t = 0; t < nb; ++t) {
        uint32_t c = 0;
        for (uint32_t w = 0; w < kMaskTileWords; ++w) c += (uint32_t)__builtin_popcountll(mask[t * kMaskTileWords + w]);
        counts[t] = c;
    }
    std::vector<uint64_t> prefix(nb + 1);
    const uint64_t total = mask_tile_prefix(counts.data(), nb, prefix.data());
    std::vector<uint64_t> ref(total + 1);
    mask_expand_range(mask.data(), n, prefix.data(), 0, nb, ref.data(), 0);
    const size_t list_bytes = std::max<size_t>((total + 8) * sizeof(uint64_t), size_t(2) << 20);

    int n_dev = 0;
    const bool device = hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0;
    std::printf("points %llu  inliers %llu  tiles %u  avx512 %d  device %d\n", (unsigned long long)n, (unsigned long long)total, nb,
                (int)mask_have_avx512(), (int)device);

    // the two destinations and the two homes of the mask
    std::vector<uint64_t> dst_pageable(total + 8);
    uint64_t *dst_lib = nullptr, *mask_pinned = nullptr, *d_mask = nullptr;
    uint32_t *counts_pinned = nullptr, *d_counts = nullptr;
    hipStream_t stream = nullptr;
    if (device) {
        dst_lib = static_cast<uint64_t*>(m3d_host_alloc(list_bytes));
        if (!dst_lib) return 2;
        if (hipHostMalloc((void**)&mask_pinned, n_words * 8, hipHostMallocPortable) != hipSuccess) return 2;
        if (hipHostMalloc((void**)&counts_pinned, nb * 4, hipHostMallocPortable) != hipSuccess) return 2;
        if (hipMalloc((void**)&d_mask, n_words * 8) != hipSuccess || hipMalloc((void**)&d_counts, nb * 4) != hipSuccess) return 2;
        if (hipMemcpy(d_mask, mask.data(), n_words * 8, hipMemcpyHostToDevice) != hipSuccess) return 2;
        if (hipMemcpy(d_counts, counts.data(), nb * 4, hipMemcpyHostToDevice) != hipSuccess) return 2;
        if (hipStreamCreate(&stream) != hipSuccess) return 2;
    }
    struct Dest { const char* name; uint64_t* p; };
    std::vector<Dest> dests = {{"pageable", dst_pageable.data()}};
    if (device) dests.push_back({"m3d_host_alloc", dst_lib});

    const int reps = 200, read_reps = 40;
    std::printf("%-15s %-9s %-5s %-7s %2s  %8s %8s %8s  %8s\n", "destination", "mask", "pool", "split", "w", "median", "p10", "p90", "read");
    for (uint32_t writers : {8u, 12u}) {
        for (const Dest& d : dests)
            for (int dev_mask = 0; dev_mask <= (device ? 1 : 0); ++dev_mask)
                for (int pool = 0; pool <= 1; ++pool)
                    for (int form : {(int)kTiles, (int)kSpans}) {
                        if (pool && form == kTiles) continue;   // (the pool writes spans)
                        const uint64_t* m = dev_mask ? mask_pinned : mask.data();
                        const uint32_t* c = dev_mask ? counts_pinned : counts.data();
                        const Job job{m, c, n, nb, d.p, prefix.data(), form};
                        std::unique_ptr<OwnWriters> own(pool ? nullptr : new OwnWriters(writers));   // (never spinning beside the pool)
                        std::vector<double> us, rd;
                        volatile uint64_t sink = 0;
                        bool ok = true;
                        for (int r = 0; r < reps + read_reps; ++r) {
                            if (pool) MaskPool::get().arm(writers, 2000);   // (as the library: when the device work is queued)
                            if (dev_mask) {
                                copy_words_k<<<(n_words + 255) / 256, 256, 0, stream>>>(d_mask, mask_pinned, n_words);
                                copy_words_k<<<(nb / 2 + 255) / 256, 256, 0, stream>>>((const uint64_t*)d_counts, (uint64_t*)counts_pinned, nb / 2);
                                if (hipStreamSynchronize(stream) != hipSuccess) return 3;
                                if (nb & 1) counts_pinned[nb - 1] = counts[nb - 1];
                            }
                            const auto t0 = Clock::now();
                            if (pool) ok = MaskPool::get().expand(m, n, c, d.p, writers) && ok;
                            else own->expand(job);
                            const auto t1 = Clock::now();
                            if (r < reps) {
                                us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
                            } else {
                                uint64_t s = 0;
                                for (uint64_t i = 0; i < total; ++i) s += d.p[i];
                                sink = s;
                                rd.push_back(std::chrono::duration<double, std::micro>(Clock::now() - t1).count());
                            }
                        }
                        (void)sink;
                        ok = ok && std::equal(ref.begin(), ref.begin() + total, d.p);
                        std::sort(us.begin(), us.end());
                        std::sort(rd.begin(), rd.end());
                        std::printf("%-15s %-9s %-5s %-7s %2u  %8.1f %8.1f %8.1f  %8.1f  %s\n", d.name, dev_mask ? "device" : "host",
                                    pool ? "pool" : "own", form_name(form), writers, us[reps / 2], us[reps / 10], us[reps * 9 / 10],
                                    rd[read_reps / 2], ok ? "ok" : "MISMATCH");
                        std::fflush(stdout);
                    }
    }
    if (device) {
        m3d_host_free(dst_lib);
        (void)hipHostFree(mask_pinned);
        (void)hipHostFree(counts_pinned);
        (void)hipFree(d_mask);
        (void)hipFree(d_counts);
        (void)hipStreamDestroy(stream);
    }
    return 0;
}
