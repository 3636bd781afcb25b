/* knn_ref.c -- a plain-C restatement of the KNearestSearch contract (include/misc3d_amd.h, next to m3d_knn_search), the
 * oracle of tests/test_knn.py and tests/test_gpu_knn.py.  Built with gcc -O2 -ffp-contract=off (tests/knn_ref_util.py).
 *
 * d2 = serial fp64 sum over k of (q[k] - r[k])^2 from +0.0; order by (d2, index), a NaN d2 after +inf and returned as the
 * quiet NaN 0x7FF8000000000000; kout = min(knn, n); dist = sqrt(max(d2, 0)); hybrid: i = first position with
 * dist > radius (or kout), num = i - 1 kept, count -1 where the reference's size_t wraps (i == 0). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    uint64_t key;
    uint32_t idx;
} pair_t;

static uint64_t key_of(double d2) {
    uint64_t k;
    if (d2 != d2) return 0x7FF8000000000000ull;
    memcpy(&k, &d2, 8);
    return k;
}
static double d2_of(uint64_t k) {
    double d;
    memcpy(&d, &k, 8);
    return d;
}
static int less(pair_t a, pair_t b) { return a.key < b.key || (a.key == b.key && a.idx < b.idx); }
static int cmp(const void* x, const void* y) {
    const pair_t a = *(const pair_t*)x, b = *(const pair_t*)y;
    return less(a, b) ? -1 : (less(b, a) ? 1 : 0);
}

double knn_ref_d2(const double* q, const double* r, int dim) {
    double acc = 0.0;
    for (int k = 0; k < dim; ++k) {
        const double d = q[k] - r[k];
        const double sq = d * d;
        acc = acc + sq;
    }
    return acc;
}

/* data: n rows of dim doubles; queries: m rows.  Outputs m x kout (kout = min(knn, n)) row-major, padded -1 / +inf. */
void knn_ref_search(const double* data, size_t n, int dim, const double* queries, size_t m, int search, int64_t knn,
                    double radius, int64_t* idx, double* dist, double* d2, int64_t* counts) {
    const size_t kout = (size_t)knn < n ? (size_t)knn : n;
    pair_t* all = (pair_t*)malloc(sizeof(pair_t) * (n ? n : 1));
    pair_t* best = (pair_t*)malloc(sizeof(pair_t) * (kout ? kout : 1));
    for (size_t q = 0; q < m; ++q) {
        const double* qv = queries + q * (size_t)dim;
        size_t got = 0;
        if (kout <= 256) {   /* insertion into a sorted list of kout */
            for (size_t r = 0; r < n && kout; ++r) {
                pair_t p = {key_of(knn_ref_d2(qv, data + r * (size_t)dim, dim)), (uint32_t)r};
                if (got == kout && !less(p, best[kout - 1])) continue;
                size_t j = got < kout ? got++ : kout - 1;
                while (j > 0 && less(p, best[j - 1])) {
                    best[j] = best[j - 1];
                    --j;
                }
                best[j] = p;
            }
        } else {
            for (size_t r = 0; r < n; ++r) {
                all[r].key = key_of(knn_ref_d2(qv, data + r * (size_t)dim, dim));
                all[r].idx = (uint32_t)r;
            }
            qsort(all, n, sizeof(pair_t), cmp);
            memcpy(best, all, sizeof(pair_t) * kout);
        }
        int64_t* iq = idx + q * kout;
        double* dq = dist + q * kout;
        double* d2q = d2 + q * kout;
        for (size_t j = 0; j < kout; ++j) {
            const double v = d2_of(best[j].key);
            iq[j] = best[j].idx;
            d2q[j] = v;
            dq[j] = v != v ? v : sqrt(v < 0.0 ? 0.0 : v);
        }
        if (search == 0) {
            counts[q] = (int64_t)kout;
            continue;
        }
        size_t i = 0;
        while (i < kout && !(dq[i] > radius)) ++i;
        const int64_t num = (int64_t)i - 1;
        counts[q] = num;
        for (size_t j = num > 0 ? (size_t)num : 0; j < kout; ++j) {
            iq[j] = -1;
            dq[j] = INFINITY;
            d2q[j] = INFINITY;
        }
    }
    free(all);
    free(best);
}
