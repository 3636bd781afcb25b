// m3d_mask_expand.hpp -- an inlier bit mask (bit i of word i / 64 = point i, creation order) -> the ascending index list.
// Header-only and free of HIP: the library's RefineModel path (m3d_refine.cpp) and the CPU tests / microbenchmark
// (tests/test_inlier_mask_expand.py, tools/ubench/expand_mask.cpp) compile the same code.
//
// The device ships the mask (1 bit per point) and one count per tile of kMaskTileWords words; the host writes the 8-byte
// indices itself.  The tiles are cut into ranges of about equal OUTPUT length; a writer of range [t0, t1) stores exactly the
// entries [prefix[t0], prefix[t1]) and never one outside them -- so writers may run side by side on one destination, and
// nothing is written at or past the list's end.  A mask word whose bits disagree with its tile's count is an error (false),
// detected before a store could leave the range.
//
// The library's pool (m3d_mask_pool.hpp) cuts the LIST, not the tiles: spans of entries [p0, p1) whose first entries fall on
// 64-byte lines of the destination (mask_split_lines, mask_expand_span), so that no line is written by two writers.  The same
// rules hold for a span: a tile is compared with its count before an entry of it is stored, and no store leaves the span.
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
__attribute__((always_inline)) inline uint64_t word_at(const uint64_t* mask, uint64_t w, uint64_t n) {
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

// ---- spans: a writer's share as entries [p0, p1) of the list, not as whole tiles, so that a share can begin on a 64-byte line
// of the destination.  A tile is compared with its count BEFORE an entry of it is stored; after that every position is known
// from the mask alone, and the words at a span's two ends are cut to the span's own bits.

// tile t's words [w0, w1) and whether their set bits agree with the tile's count
__attribute__((always_inline)) inline bool tile_agrees(const uint64_t* mask, uint64_t n, const uint64_t* prefix, uint32_t t, uint64_t* w0, uint64_t* w1) {
    const uint64_t n_words = (n + 63) / 64;
    *w0 = (uint64_t)t * kMaskTileWords;
    *w1 = *w0 + kMaskTileWords < n_words ? *w0 + kMaskTileWords : n_words;
    uint64_t c = 0;
    for (uint64_t w = *w0; w < *w1; ++w) c += (uint64_t)__builtin_popcountll(word_at(mask, w, n));
    return c == prefix[t + 1] - prefix[t];
}
// the first tile whose entries end behind position p (tiles of count 0 are passed over)
inline uint32_t tile_of(const uint64_t* prefix, uint32_t nb, uint64_t p) {
    uint32_t lo = 0, hi = nb;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (prefix[mid + 1] > p) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// word m without its `skip` lowest set bits, and with no more than `room` set bits left (the lowest ones)
__attribute__((always_inline)) inline uint64_t cut_word(uint64_t m, uint64_t skip, uint64_t room) {
    for (; skip && m; --skip) m &= m - 1;
    while (m && (uint64_t)__builtin_popcountll(m) > room) m &= ~(1ull << (63 - __builtin_clzll(m)));
    return m;
}

// The tiles that hold entries [p0, p1), one per next(), each compared with its count first.  (A cursor and not a callback: the
// AVX-512 writers below inline it, and a lambda would not carry their target attribute.)
struct SpanTiles {
    const uint64_t* mask;
    uint64_t n;
    const uint64_t* prefix;
    uint32_t nb;
    uint64_t p0, p1;
    uint32_t t;       // the next tile to open
    bool ok = true;   // false: a tile disagreed with its count, or the span ends behind the list
    SpanTiles(const uint64_t* mask_, uint64_t n_, const uint64_t* prefix_, uint32_t nb_, uint64_t p0_, uint64_t p1_)
        : mask(mask_), n(n_), prefix(prefix_), nb(nb_), p0(p0_), p1(p1_), t(nb_) {
        if (p0 >= p1) return;
        if (p1 > prefix[nb]) {
            ok = false;
            return;
        }
        t = tile_of(prefix, nb, p0);
        if (prefix[t] == p0)   // tiles of count 0 that sit at the span's first entry are this span's to check
            while (t > 0 && prefix[t - 1] == p0) --t;
    }
    // the tile's words [w0, w1), the position of its first entry, whether all its entries are the span's; false: the span is
    // written (or !ok).  A tile of count 0 whose place in the list is inside the span -- or at the list's end, for the span that
    // ends there -- is compared with its count like every other and then passed over: every tile is some span's, unless the list
    // is empty (no span stores anything then, and the caller's own total says so).
    __attribute__((always_inline)) inline bool next(uint64_t* w0, uint64_t* w1, uint64_t* first, bool* whole) {
        for (;;) {
            if (t >= nb) return false;
            const bool empty = prefix[t + 1] == prefix[t];
            if (prefix[t] >= p1 && !(empty && p1 == prefix[nb])) return false;
            if (!tile_agrees(mask, n, prefix, t, w0, w1)) {
                ok = false;
                return false;
            }
            ++t;
            if (empty) continue;
            *first = prefix[t - 1];
            *whole = prefix[t - 1] >= p0 && prefix[t] <= p1;
            return true;
        }
    }
    // a word of a tile that is not whole: its bits inside the span (0: none), *pos moved from its first entry to the first kept,
    // *after to the word's end
    __attribute__((always_inline)) inline uint64_t cut(uint64_t m, uint64_t* pos, uint64_t* after) const {
        const uint64_t first = *pos, pc = (uint64_t)__builtin_popcountll(m);
        *after = first + pc;
        if (first + pc <= p0 || first >= p1) return 0;
        const uint64_t skip = first < p0 ? p0 - first : 0;
        *pos = first + skip;
        return (skip || first + pc > p1) ? cut_word(m, skip, p1 - (first + skip)) : m;
    }
};

inline bool span_scalar(const uint64_t* mask, uint64_t n, const uint64_t* prefix, uint32_t nb, uint64_t p0, uint64_t p1, uint64_t* dst) {
    SpanTiles tiles(mask, n, prefix, nb, p0, p1);
    uint64_t w0, w1, pos;
    bool whole;
    while (tiles.next(&w0, &w1, &pos, &whole))
        for (uint64_t w = w0; w < w1; ++w) {
            uint64_t m = word_at(mask, w, n);
            if (!m) continue;
            uint64_t after = 0;
            if (!whole) m = tiles.cut(m, &pos, &after);
            for (const uint64_t b = w * 64; m; m &= m - 1) dst[pos++] = b + (uint64_t)__builtin_ctzll(m);
            if (!whole) pos = after;
        }
    return tiles.ok;
}

#if defined(__x86_64__)
// one compress and one masked, unaligned store per 8-bit slice, as expand_avx512 above
__attribute__((target("avx512f,popcnt"))) inline bool span_avx512_masked(const uint64_t* mask, uint64_t n, const uint64_t* prefix,
                                                                         uint32_t nb, uint64_t p0, uint64_t p1, uint64_t* dst) {
    const __m512i lane = _mm512_set_epi64(7, 6, 5, 4, 3, 2, 1, 0);
    const __m512i eight = _mm512_set1_epi64(8);
    SpanTiles tiles(mask, n, prefix, nb, p0, p1);
    uint64_t w0, w1, pos;
    bool whole;
    while (tiles.next(&w0, &w1, &pos, &whole))
        for (uint64_t w = w0; w < w1; ++w) {
            uint64_t m = word_at(mask, w, n);
            if (!m) continue;
            uint64_t after = 0;
            if (!whole) {
                m = tiles.cut(m, &pos, &after);
                if (!m) {
                    pos = after;
                    continue;
                }
            }
            __m512i v = _mm512_add_epi64(_mm512_set1_epi64((long long)(w * 64)), lane);
            uint64_t* d = dst + pos;
            if (m == ~0ull) {
                for (int k = 0; k < 8; ++k) {
                    _mm512_storeu_si512(d, v);
                    d += 8;
                    v = _mm512_add_epi64(v, eight);
                }
            } else {
                for (int k = 0; k < 8; ++k) {
                    const __mmask8 s = (__mmask8)(m >> (8 * k));
                    if (s) {
                        const unsigned c_n = (unsigned)_mm_popcnt_u32(s);
                        _mm512_mask_storeu_epi64(d, (__mmask8)((1u << c_n) - 1u), _mm512_maskz_compress_epi64(s, v));
                        d += c_n;
                    }
                    v = _mm512_add_epi64(v, eight);
                }
            }
            pos = whole ? (uint64_t)(d - dst) : after;
        }
    return tiles.ok;
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

// cut the list [0, total) into `parts` spans of about equal length: cuts[0] = 0 ... cuts[parts] = total, every cut between them
// rounded to the nearest entry that begins a 64-byte line of dst -- no line of the destination is shared by two writers
// except where a span is empty
inline void mask_split_lines(uint64_t total, uint32_t parts, const uint64_t* dst, uint64_t* cuts) {
    const uint64_t a = ((uintptr_t)dst >> 3) & 7u;   // dst[0] is entry `a` of its line
    cuts[0] = 0;
    for (uint32_t k = 1; k < parts; ++k) {
        uint64_t c = (total * k / parts + a + 4) & ~7ull;
        c = c > a ? c - a : 0;
        if (c > total) c = total;
        cuts[k] = c < cuts[k - 1] ? cuts[k - 1] : c;
    }
    cuts[parts] = total;
}

// entries [p0, p1) of the list of a mask of n points (nb tiles, prefix[nb] = total) into dst[p0, p1): nothing is stored outside
// them.  false: a tile the span touches disagrees with its count (no entry of that tile was stored), or p1 > total.
inline bool mask_expand_span(const uint64_t* mask, uint64_t n, const uint64_t* prefix, uint32_t nb, uint64_t p0, uint64_t p1,
                             uint64_t* dst, int path = -1) {
#if defined(__x86_64__)
    if (path != 0 && mask_have_avx512()) return mask_detail::span_avx512_masked(mask, n, prefix, nb, p0, p1, dst);
#endif
    return mask_detail::span_scalar(mask, n, prefix, nb, p0, p1, dst);
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

// the same by spans of the list that begin on lines of dst (mask_split_lines, mask_expand_span)
inline bool mask_expand_spans_threads(const uint64_t* mask, uint64_t n, const uint32_t* counts, uint64_t* dst, uint32_t writers,
                                      int path = -1) {
    const uint32_t nb = (uint32_t)((n + 64ull * kMaskTileWords - 1) / (64ull * kMaskTileWords));
    if (writers < 1) writers = 1;
    std::vector<uint64_t> prefix(nb + 1);
    const uint64_t total = mask_tile_prefix(counts, nb, prefix.data());
    std::vector<uint64_t> cuts(writers + 1);
    mask_split_lines(total, writers, dst, cuts.data());
    std::vector<char> ok(writers, 1);
    std::vector<std::thread> th;
    for (uint32_t k = 1; k < writers; ++k)
        th.emplace_back([&, k] { ok[k] = mask_expand_span(mask, n, prefix.data(), nb, cuts[k], cuts[k + 1], dst, path); });
    ok[0] = mask_expand_span(mask, n, prefix.data(), nb, cuts[0], cuts[1], dst, path);
    for (auto& t : th) t.join();
    for (char c : ok)
        if (!c) return false;
    return true;
}

}  // namespace m3d
