// m3d_mask_expand.hpp -- an inlier bit mask (bit i of word i / 64 = point i, creation order) -> the ascending index list.
// Header-only and free of HIP: the library's RefineModel path (m3d_refine.cpp) and the CPU tests / microbenchmark
// (tests/test_inlier_mask_expand.py, tools/ubench/expand_mask.cpp) compile the same code.
//
// The device ships the mask (1 bit per point) and one count per tile of kMaskTileWords words; the host writes the 8-byte
// indices itself.  The tiles are cut into ranges of about equal OUTPUT length; a writer of range [t0, t1) stores exactly the
// entries [prefix[t0], prefix[t1]) and never one outside them -- so writers may run side by side on one destination, and
// nothing is written at or past the list's end.  A mask word whose bits disagree with its tile's count is an error (false),
// detected before a store could leave the range.
#pragma once

#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace m3d {

constexpr uint32_t kMaskTileWords = 32;   // 2048 points: one compaction workgroup's tile (kCompactTile)

// exclusive prefix of the tile counts; prefix[nb] = total
inline uint64_t mask_tile_prefix(const uint32_t* counts, uint32_t nb, uint64_t* prefix) {
    uint64_t s = 0;
    for (uint32_t t = 0; t < nb; ++t) {
        prefix[t] = s;
        s += counts[t];
    }
    prefix[nb] = s;
    return s;
}

// cut [0, nb) into `parts` contiguous tile ranges of about equal output length: bounds[0] = 0 ... bounds[parts] = nb
inline void mask_split(const uint64_t* prefix, uint32_t nb, uint32_t parts, uint32_t* bounds) {
    const uint64_t total = prefix[nb];
    bounds[0] = 0;
    uint32_t t = 0;
    for (uint32_t k = 1; k < parts; ++k) {
        const uint64_t want = total * k / parts;
        while (t < nb && prefix[t] < want) ++t;
        bounds[k] = t;
    }
    bounds[parts] = nb;
}

namespace mask_detail {

// the last word's bits at or past n (none are set by the device; masked here so that a stray one cannot index past n)
inline uint64_t word_at(const uint64_t* mask, uint64_t w, uint64_t n) {
    const uint64_t m = mask[w];
    const uint64_t first = w * 64;
    return n - first >= 64 ? m : (m & ((1ull << (n - first)) - 1ull));
}

inline bool expand_scalar(const uint64_t* mask, uint64_t n, const uint64_t* prefix, uint32_t t0, uint32_t t1, uint64_t* dst) {
    const uint64_t n_words = (n + 63) / 64;
    for (uint32_t t = t0; t < t1; ++t) {
        uint64_t pos = prefix[t];
        const uint64_t end = prefix[t + 1];
        const uint64_t w0 = (uint64_t)t * kMaskTileWords, w1 = w0 + kMaskTileWords < n_words ? w0 + kMaskTileWords : n_words;
        for (uint64_t w = w0; w < w1; ++w) {
            uint64_t m = word_at(mask, w, n);
            if (!m) continue;
            if (pos + (uint64_t)__builtin_popcountll(m) > end) return false;
            const uint64_t b = w * 64;
            do {
                dst[pos++] = b + (uint64_t)__builtin_ctzll(m);
                m &= m - 1;
            } while (m);
        }
        if (pos != end) return false;
    }
    return true;
}

#if defined(__x86_64__)
// eight indices per 8-bit slice: a compress in the register, then a store masked to the slice's popcount (a full-vector store
// would run into the next writer's entries; vpcompressq to memory is microcoded on some cores)
__attribute__((target("avx512f,popcnt"))) inline bool expand_avx512(const uint64_t* mask, uint64_t n, const uint64_t* prefix,
                                                                uint32_t t0, uint32_t t1, uint64_t* dst) {
    const uint64_t n_words = (n + 63) / 64;
    const __m512i lane = _mm512_set_epi64(7, 6, 5, 4, 3, 2, 1, 0);
    const __m512i eight = _mm512_set1_epi64(8);
    for (uint32_t t = t0; t < t1; ++t) {
        uint64_t pos = prefix[t];
        const uint64_t end = prefix[t + 1];
        const uint64_t w0 = (uint64_t)t * kMaskTileWords, w1 = w0 + kMaskTileWords < n_words ? w0 + kMaskTileWords : n_words;
        for (uint64_t w = w0; w < w1; ++w) {
            const uint64_t m = word_at(mask, w, n);
            if (!m) continue;
            const uint64_t pc = (uint64_t)_mm_popcnt_u64(m);
            if (pos + pc > end) return false;
            __m512i v = _mm512_add_epi64(_mm512_set1_epi64((long long)(w * 64)), lane);
            uint64_t* d = dst + pos;
            if (m == ~0ull) {   // a word of inliers only: 64 consecutive indices
                for (int k = 0; k < 8; ++k) {
                    _mm512_storeu_si512(d + 8 * k, v);
                    v = _mm512_add_epi64(v, eight);
                }
            } else {
                for (int k = 0; k < 8; ++k) {
                    const __mmask8 s = (__mmask8)(m >> (8 * k));
                    if (s) {
                        const __m512i c = _mm512_maskz_compress_epi64(s, v);
                        const unsigned c_n = (unsigned)_mm_popcnt_u32(s);
                        _mm512_mask_storeu_epi64(d, (__mmask8)((1u << c_n) - 1u), c);
                        d += c_n;
                    }
                    v = _mm512_add_epi64(v, eight);
                }
            }
            pos += pc;
        }
        if (pos != end) return false;
    }
    return true;
}
#endif

}  // namespace mask_detail

inline bool mask_have_avx512() {
#if defined(__x86_64__)
    static const bool have = __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("popcnt");
    return have;
#else
    return false;
#endif
}

// tiles [t0, t1) of a mask of n points into dst[prefix[t0], prefix[t1]); false: a word's bits disagree with the counts.
// path: 0 the portable loop, 1 AVX-512 where the CPU has it (-1, default: the same)
inline bool mask_expand_range(const uint64_t* mask, uint64_t n, const uint64_t* prefix, uint32_t t0, uint32_t t1, uint64_t* dst,
                              int path = -1) {
#if defined(__x86_64__)
    if (path != 0 && mask_have_avx512()) return mask_detail::expand_avx512(mask, n, prefix, t0, t1, dst);
#endif
    return mask_detail::expand_scalar(mask, n, prefix, t0, t1, dst);
}

// the whole list by `writers` threads (the calling one among them), started for this call: for the tests and the
// microbenchmark -- the library keeps its writers alive between calls (m3d_refine.cpp)
inline bool mask_expand_threads(const uint64_t* mask, uint64_t n, const uint32_t* counts, uint64_t* dst, uint32_t writers,
                                int path = -1) {
    const uint32_t nb = (uint32_t)((n + 64ull * kMaskTileWords - 1) / (64ull * kMaskTileWords));
    if (writers < 1) writers = 1;
    std::vector<uint64_t> prefix(nb + 1);
    mask_tile_prefix(counts, nb, prefix.data());
    std::vector<uint32_t> bounds(writers + 1);
    mask_split(prefix.data(), nb, writers, bounds.data());
    std::vector<char> ok(writers, 1);
    std::vector<std::thread> th;
    for (uint32_t k = 1; k < writers; ++k)
        th.emplace_back([&, k] { ok[k] = mask_expand_range(mask, n, prefix.data(), bounds[k], bounds[k + 1], dst, path); });
    ok[0] = mask_expand_range(mask, n, prefix.data(), bounds[0], bounds[1], dst, path);
    for (auto& t : th) t.join();
    for (char c : ok)
        if (!c) return false;
    return true;
}

}  // namespace m3d
