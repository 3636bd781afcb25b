/* ppf_train_ref.c -- the contract "PPF model preprocessing" of include/misc3d_amd.h in serial C, written the way the reference
 * runs it: the priority-queue walk with the O2 order for the orientation, the FIFO walk for the sampler, both over brute-force
 * neighbourhoods, B1 / B2 / B4, and SampleWithoutDuplicate over its own mt19937.  Built by tests/ppf_train_ref_util.py with
 * gcc -O2 -ffp-contract=off; shares no code with the library. */
#define _POSIX_C_SOURCE 199309L
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

static double d2_of(const double *a, const double *b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}
#if defined(PTR_FP_ORDER) && PTR_FP_ORDER == 1
static double dot3(const double *a, const double *b) { return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2]); }
#else
static double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
#endif

/* ---- brute-force radius lists: for every point the others with d2 < r2, ascending (d2, index) */
typedef struct {
    double d2;
    uint32_t j;
} nb_t;
static int nb_cmp(const void *a, const void *b) {
    const nb_t *x = (const nb_t *)a, *y = (const nb_t *)b;
    if (x->d2 != y->d2) return x->d2 < y->d2 ? -1 : 1;
    return x->j < y->j ? -1 : (x->j > y->j ? 1 : 0);
}
typedef struct {
    size_t *off;
    nb_t *nb;
} lists_t;
static lists_t lists_build(const double *xyz, size_t n, double r2) {
    lists_t L;
    L.off = (size_t *)calloc(n + 1, sizeof(size_t));
    size_t cap = 16 * n + 16, m = 0;
    L.nb = (nb_t *)malloc(cap * sizeof(nb_t));
    for (size_t i = 0; i < n; ++i) {
        L.off[i] = m;
        for (size_t j = 0; j < n; ++j) {
            if (j == i) continue;
            const double d2 = d2_of(xyz + 3 * i, xyz + 3 * j);
            if (!(d2 < r2)) continue;
            if (m == cap) L.nb = (nb_t *)realloc(L.nb, (cap *= 2) * sizeof(nb_t));
            L.nb[m].d2 = d2;
            L.nb[m++].j = (uint32_t)j;
        }
        qsort(L.nb + L.off[i], m - L.off[i], sizeof(nb_t), nb_cmp);
    }
    L.off[n] = m;
    return L;
}
static void lists_free(lists_t *L) {
    free(L->off);
    free(L->nb);
}

/* ---- the heap of the walk: (d2, lo, hi) ascending, the point to visit as payload */
typedef struct {
    double d2;
    uint32_t lo, hi, to;
} he_t;
static int he_less(const he_t *a, const he_t *b) {
    if (a->d2 != b->d2) return a->d2 < b->d2;
    if (a->lo != b->lo) return a->lo < b->lo;
    return a->hi < b->hi;
}
typedef struct {
    he_t *a;
    size_t n, cap;
} heap_t;
static void heap_push(heap_t *h, he_t e) {
    if (h->n == h->cap) h->a = (he_t *)realloc(h->a, (h->cap = h->cap ? 2 * h->cap : 1024) * sizeof(he_t));
    size_t i = h->n++;
    while (i && he_less(&e, &h->a[(i - 1) / 2])) {
        h->a[i] = h->a[(i - 1) / 2];
        i = (i - 1) / 2;
    }
    h->a[i] = e;
}
static he_t heap_pop(heap_t *h) {
    const he_t top = h->a[0], e = h->a[--h->n];
    size_t i = 0;
    for (;;) {
        size_t c = 2 * i + 1;
        if (c >= h->n) break;
        if (c + 1 < h->n && he_less(&h->a[c + 1], &h->a[c])) ++c;
        if (!he_less(&h->a[c], &e)) break;
        h->a[i] = h->a[c];
        i = c;
    }
    if (h->n) h->a[i] = e;
    return top;
}

static uint32_t uf_find(uint32_t *p, uint32_t x) {
    while (p[x] != x) x = p[x] = p[p[x]];
    return x;
}

/* O5's rounds: Boruvka over the lists with the driver's stopping rule; *forest = the edges of the whole forest */
static uint64_t boruvka_rounds(const lists_t *L, size_t n, uint64_t *forest) {
    uint32_t *p = (uint32_t *)malloc(n * sizeof(uint32_t)), *label = (uint32_t *)malloc(n * sizeof(uint32_t));
    he_t *best = (he_t *)malloc(n * sizeof(he_t));
    char *has = (char *)malloc(n);
    for (size_t i = 0; i < n; ++i) p[i] = (uint32_t)i;
    uint64_t rounds = 0, have = 0;
    for (;;) {
        for (size_t i = 0; i < n; ++i) label[i] = uf_find(p, (uint32_t)i);
        memset(has, 0, n);
        for (size_t i = 0; i < n; ++i)
            for (size_t k = L->off[i]; k < L->off[i + 1]; ++k) {
                const uint32_t j = L->nb[k].j;
                if (label[j] == label[i]) continue;
                he_t e = {L->nb[k].d2, (uint32_t)(i < j ? i : j), (uint32_t)(i < j ? j : i), j};
                if (!has[label[i]] || he_less(&e, &best[label[i]])) {
                    best[label[i]] = e;
                    has[label[i]] = 1;
                }
            }
        uint64_t added = 0;
        for (size_t c = 0; c < n; ++c) {
            if (!has[c]) continue;
            const uint32_t a = uf_find(p, best[c].lo), b = uf_find(p, best[c].hi);
            if (a == b) continue; /* the other end's label chose the same edge */
            p[a > b ? a : b] = a > b ? b : a;
            ++added;
        }
        ++rounds;
        have += added;
        if (!added || have == n - 1) break;
    }
    *forest = have;
    free(p);
    free(label);
    free(best);
    free(has);
    return rounds;
}

static double now_ms(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return 1e3 * (double)t.tv_sec + 1e-6 * (double)t.tv_nsec;
}

/* O1 - O5 by the reference's walk.  stats: rounds, tree_edges, component, flips.  ms (may be null): the brute-force lists, the
 * walk itself (heap, flips), the Boruvka count of O5's rounds; edges (may be null): the directed entries of the lists */
void ptr_orient_timed(const double *xyz, const double *normals, size_t n, double radius, size_t seed, double *out, int64_t *parent,
                      uint64_t *stats, double *ms, uint64_t *edges) {
    const double t0 = now_ms();
    lists_t L = lists_build(xyz, n, radius * radius);
    const double t1 = now_ms();
    char *done = (char *)calloc(n, 1);
    heap_t h = {0, 0, 0};
    memcpy(out, normals, 3 * n * sizeof(double));
    for (size_t i = 0; i < n; ++i) parent[i] = -2;
    uint64_t component = 0, flips = 0;
    he_t first = {0.0, (uint32_t)seed, (uint32_t)seed, (uint32_t)seed};
    heap_push(&h, first);
    while (h.n) {
        const uint32_t cur = heap_pop(&h).to;
        if (done[cur]) continue;
        for (size_t k = L.off[cur]; k < L.off[cur + 1]; ++k) {
            const uint32_t j = L.nb[k].j;
            if (done[j]) continue;
            he_t e = {L.nb[k].d2, cur < j ? cur : j, cur < j ? j : cur, j};
            heap_push(&h, e);
        }
        parent[cur] = -1;
        for (size_t k = L.off[cur]; k < L.off[cur + 1]; ++k) {
            const uint32_t j = L.nb[k].j;
            if (!done[j]) continue;
            parent[cur] = j; /* the first done neighbour; its normal is final */
            if (dot3(out + 3 * cur, out + 3 * j) < 0.0) {
                for (int a = 0; a < 3; ++a) out[3 * cur + a] = -out[3 * cur + a];
                ++flips;
            }
            break;
        }
        done[cur] = 1;
        ++component;
    }
    const double t2 = now_ms();
    stats[0] = boruvka_rounds(&L, n, &stats[1]);
    if (ms) ms[0] = t1 - t0, ms[1] = t2 - t1, ms[2] = now_ms() - t2;
    if (edges) *edges = (uint64_t)L.off[n];
    stats[2] = component;
    stats[3] = flips;
    free(h.a);
    free(done);
    lists_free(&L);
}
void ptr_orient(const double *xyz, const double *normals, size_t n, double radius, size_t seed, double *out, int64_t *parent,
                uint64_t *stats) {
    ptr_orient_timed(xyz, normals, n, radius, seed, out, parent, stats, 0, 0);
}

/* B5: S(step) by the FIFO walk over brute-force neighbourhoods -> the number selected */
size_t ptr_sample(const double *xyz, size_t n, double step, size_t seed, size_t *out) {
    const double search_r = step * 2, r2 = search_r * search_r;
    char *checked = (char *)calloc(n, 1);
    size_t qcap = 4 * n + 16, qh = 0, qt = 0, k = 0;
    uint32_t *q = (uint32_t *)malloc(qcap * sizeof(uint32_t));
    nb_t *near = (nb_t *)malloc(n * sizeof(nb_t));
    q[qt++] = (uint32_t)seed;
    while (qh < qt) {
        const uint32_t cur = q[qh++];
        if (checked[cur]) continue;
        checked[cur] = 1;
        out[k++] = cur;
        size_t m = 0;
        for (size_t j = 0; j < n; ++j) {
            const double d2 = d2_of(xyz + 3 * cur, xyz + 3 * j);
            if (d2 < r2) {
                near[m].d2 = d2;
                near[m++].j = (uint32_t)j;
            }
        }
        qsort(near, m, sizeof(nb_t), nb_cmp);
        for (size_t i = 0; i < m; ++i) {
            if (checked[near[i].j]) continue;
            if (sqrt(near[i].d2) < step) {
                checked[near[i].j] = 1;
            } else {
                if (qt == qcap) q = (uint32_t *)realloc(q, (qcap *= 2) * sizeof(uint32_t));
                q[qt++] = near[i].j;
            }
        }
    }
    free(checked);
    free(q);
    free(near);
    return k;
}

/* B1: cumulants, the cyclic Jacobi of the contract (pairs (0,1), (0,2), (1,2), at most 24 sweeps), extents in that frame */
void ptr_box(const double *xyz, size_t n, double *center, double *extent) {
    double c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < n; ++i) {
        const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        c[0] += x, c[1] += y, c[2] += z;
        c[3] += x * x, c[4] += x * y, c[5] += x * z, c[6] += y * y, c[7] += y * z, c[8] += z * z;
    }
    for (int k = 0; k < 9; ++k) c[k] /= (double)n;
    double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    A[0][0] = c[3] - c[0] * c[0], A[1][1] = c[6] - c[1] * c[1], A[2][2] = c[8] - c[2] * c[2];
    A[0][1] = A[1][0] = c[4] - c[0] * c[1];
    A[0][2] = A[2][0] = c[5] - c[0] * c[2];
    A[1][2] = A[2][1] = c[7] - c[1] * c[2];
    static const int P[3] = {0, 0, 1}, Q[3] = {1, 2, 2};
    for (int sweep = 0; sweep < 24; ++sweep) {
        if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[1][2] == 0.0) break;
        for (int e = 0; e < 3; ++e) {
            const int p = P[e], q = Q[e];
            const double apq = A[p][q];
            if (apq == 0.0) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
            for (int k = 0; k < 3; ++k) {
                const double akp = A[k][p], akq = A[k][q];
                A[k][p] = cs * akp - sn * akq;
                A[k][q] = sn * akp + cs * akq;
            }
            for (int k = 0; k < 3; ++k) {
                const double apk = A[p][k], aqk = A[q][k];
                A[p][k] = cs * apk - sn * aqk;
                A[q][k] = sn * apk + cs * aqk;
            }
            A[p][q] = A[q][p] = 0.0;
            for (int k = 0; k < 3; ++k) {
                const double vkp = V[k][p], vkq = V[k][q];
                V[k][p] = cs * vkp - sn * vkq;
                V[k][q] = sn * vkp + cs * vkq;
            }
        }
    }
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (size_t i = 0; i < n; ++i) {
        const double d[3] = {xyz[3 * i] - c[0], xyz[3 * i + 1] - c[1], xyz[3 * i + 2] - c[2]};
        for (int k = 0; k < 3; ++k) {
            const double ax[3] = {V[0][k], V[1][k], V[2][k]};
            const double v = dot3(ax, d);
            if (i == 0 || v < lo[k]) lo[k] = v;
            if (i == 0 || v > hi[k]) hi[k] = v;
        }
    }
    double mid[3];
    for (int k = 0; k < 3; ++k) {
        extent[k] = hi[k] - lo[k];
        mid[k] = (hi[k] + lo[k]) * 0.5;
    }
    for (int r = 0; r < 3; ++r) center[r] = c[r] + ((V[r][0] * mid[0] + V[r][1] * mid[1]) + V[r][2] * mid[2]);
}

/* B2 -> out: diameter, r_min, dist_step, dist_step_dense, normal_r, view_pt[3] */
void ptr_derive(const double *center, const double *extent, double rel_sample, double rel_dense, double normal_rel, double *out) {
    const double *d = extent;
    double o[3] = {d[0], d[1], d[2]};
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2 - i; ++j)
            if (o[j + 1] < o[j]) {
                const double t = o[j];
                o[j] = o[j + 1];
                o[j + 1] = t;
            }
    out[0] = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    out[1] = sqrt(o[0] * o[0] + o[1] * o[1]);
    out[2] = out[0] * rel_sample;
    out[3] = out[0] * rel_dense;
    out[4] = out[0] * normal_rel;
    out[5] = center[0];
    out[6] = center[1];
    out[7] = center[2] + 2.0 * out[0];
}

/* B3 (NormalizeNormals, in place), B4 (the seed; the seed's normal flipped in place unless `keep`), O1 - O4 unless `keep`.
 * -> the seed.  info: seed_flipped, then ptr_orient's four stats */
size_t ptr_prepare_normals(const double *xyz, double *nrm, size_t n, const double *view_pt, double normal_r, int invert, int keep,
                           double *out, int64_t *parent, uint64_t *info) {
    for (size_t i = 0; i < n; ++i) {
        double *v = nrm + 3 * i;
        const double s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
        if (s > 0.0) {
            const double len = sqrt(s);
            v[0] /= len, v[1] /= len, v[2] /= len;
        }
    }
    size_t seed = 0;
    double bd = 0.0;
    for (size_t i = 0; i < n; ++i) {
        const double d2 = d2_of(view_pt, xyz + 3 * i);
        if (i == 0 || d2 < bd) seed = i, bd = d2;
    }
    memset(info, 0, 5 * sizeof(uint64_t));
    if (keep) {
        memcpy(out, nrm, 3 * n * sizeof(double));
        return seed;
    }
    const double to_view[3] = {view_pt[0] - xyz[3 * seed], view_pt[1] - xyz[3 * seed + 1], view_pt[2] - xyz[3 * seed + 2]};
    int flip = dot3(to_view, nrm + 3 * seed) < 0.0;
    if (invert) flip = !flip;
    if (flip)
        for (int a = 0; a < 3; ++a) nrm[3 * seed + a] = -nrm[3 * seed + a];
    info[0] = (uint64_t)flip;
    ptr_orient(xyz, nrm, n, normal_r, seed, out, parent, info + 1);
    return seed;
}

/* C3: std::mt19937(seed), then swap(indices[i], indices[rng() % num]) for i < sample */
void ptr_reference_indices(size_t num, size_t sample, uint32_t seed, size_t *out) {
    uint32_t mt[624];
    int pos = 624;
    mt[0] = seed;
    for (uint32_t i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + i;
    size_t *idx = (size_t *)malloc(num * sizeof(size_t));
    for (size_t i = 0; i < num; ++i) idx[i] = i;
    for (size_t i = 0; i < sample; ++i) {
        if (pos == 624) {
            for (int k = 0; k < 624; ++k) {
                const uint32_t y = (mt[k] & 0x80000000u) | (mt[(k + 1) % 624] & 0x7fffffffu);
                mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            pos = 0;
        }
        uint32_t y = mt[pos++];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= y >> 18;
        const size_t r = (size_t)y % num, t = idx[i];
        idx[i] = idx[r];
        idx[r] = t;
    }
    memcpy(out, idx, sample * sizeof(size_t));
    free(idx);
}
