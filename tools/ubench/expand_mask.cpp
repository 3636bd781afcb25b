// expand_mask.cpp -- host-only microbenchmark of the inlier-mask expansion (misc3d_amd/csrc/m3d_mask_expand.hpp): how long
// 1, 2, 4, 8, 12 writers take to write the index list of a mask, portable loop and AVX-512, with the writers kept spinning
// between repetitions (as the library's pool does) so that thread start-up is not timed.
//
//   g++ -O2 -std=c++17 -pthread -I misc3d_amd/csrc tools/ubench/expand_mask.cpp -o /tmp/expand_mask
//   /tmp/expand_mask [MASK_FILE N]
// MASK_FILE: the mask as bytes, bit i of byte i / 8 = point i (np.packbits(flags, bitorder="little")), N points.  Without
// one: a C2-like mask of 1 000 000 points -- a plane holding every other 2048-point stretch, the rest clutter (~50 %).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "m3d_mask_expand.hpp"

using namespace m3d;

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
    std::vector<uint32_t> counts(nb);
    for (uint32_t t = 0; t < nb; ++t) {
        uint32_t c = 0;
        for (uint32_t w = 0; w < kMaskTileWords; ++w) c += (uint32_t)__builtin_popcountll(mask[t * kMaskTileWords + w]);
        counts[t] = c;
    }
    std::vector<uint64_t> prefix(nb + 1);
    const uint64_t total = mask_tile_prefix(counts.data(), nb, prefix.data());
    std::vector<uint64_t> dst(total + 1), ref(total + 1);
    mask_expand_range(mask.data(), n, prefix.data(), 0, nb, ref.data(), 0);
    std::printf("points %llu  inliers %llu  tiles %u  avx512 %d\n", (unsigned long long)n, (unsigned long long)total, nb,
                (int)mask_have_avx512());
    const int reps = 200;
    for (int path = 0; path <= (mask_have_avx512() ? 1 : 0); ++path) {
        for (uint32_t writers : {1u, 2u, 4u, 8u, 12u}) {
            std::vector<uint32_t> bounds(writers + 1);
            mask_split(prefix.data(), nb, writers, bounds.data());
            std::atomic<int> go{0}, done{0};
            std::atomic<bool> quit{false};
            std::vector<std::thread> th;
            for (uint32_t k = 1; k < writers; ++k)
                th.emplace_back([&, k] {
                    int seen = 0;
                    for (;;) {
                        int g;
                        while ((g = go.load(std::memory_order_acquire)) == seen && !quit.load(std::memory_order_relaxed)) {
                        }
                        if (quit.load()) return;
                        seen = g;
                        mask_expand_range(mask.data(), n, prefix.data(), bounds[k], bounds[k + 1], dst.data(), path);
                        done.fetch_add(1, std::memory_order_release);
                    }
                });
            std::vector<double> us;
            for (int r = 0; r < reps; ++r) {
                done.store(0);
                const auto t0 = std::chrono::steady_clock::now();
                go.fetch_add(1, std::memory_order_release);
                mask_expand_range(mask.data(), n, prefix.data(), bounds[0], bounds[1], dst.data(), path);
                while (done.load(std::memory_order_acquire) != (int)writers - 1) {
                }
                us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
            }
            quit.store(true);
            for (auto& t : th) t.join();
            const bool ok = std::equal(ref.begin(), ref.begin() + total, dst.begin());
            std::sort(us.begin(), us.end());
            std::printf("%-7s writers %2u  median %7.1f us  p10 %7.1f  p90 %7.1f  %s\n", path ? "avx512" : "scalar", writers,
                        us[reps / 2], us[reps / 10], us[reps * 9 / 10], ok ? "ok" : "MISMATCH");
        }
    }
    return 0;
}
