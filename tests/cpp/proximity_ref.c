/* proximity_ref.c -- plain-C restatement of ProximityExtractor::Segment's serial semantics (src/proximity_extraction.cpp)
 * for the tests: brute-force radius lists in (d2, index) order, the seed loop from j = 1, the merge sets made symmetric
 * and closed, the max_size append quirk, the min / max filter and the sort by size with the canonical tie rule (smallest
 * member index first).  The evaluators use libm's sqrt / acos.  Built with gcc -ffp-contract=off (tests/proximity_ref_util.py). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { size_t j; double d2; } nb_t;

static int kind_g;
static double dist_g, max_angle_g;
static const double *nrm_g;

static double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

static int normals_ok(size_t i, size_t j) {
    const double angle = acos(dot3(nrm_g + 3 * i, nrm_g + 3 * j));
    if (max_angle_g >= 0.0) return angle <= max_angle_g;
    const double b = M_PI - angle;
    return (b < angle ? b : angle) <= -max_angle_g;   /* std::min(angle, M_PI - angle) */
}
static int evaluate(size_t i, size_t j, double dist) {
    if (kind_g == 1) return dist < dist_g;
    if (kind_g == 3 && dist >= dist_g) return 0;
    return normals_ok(i, j);
}

static int cmp_nb(const void *a, const void *b) {
    const nb_t *x = a, *y = b;
    if (x->d2 < y->d2) return -1;
    if (x->d2 > y->d2) return 1;
    return x->j < y->j ? -1 : (x->j > y->j);
}

typedef struct { size_t *v; size_t n, cap; } vec_t;
static void push(vec_t *v, size_t x) {
    if (v->n == v->cap) {
        v->cap = v->cap ? 2 * v->cap : 4;
        v->v = realloc(v->v, v->cap * sizeof(size_t));
    }
    v->v[v->n++] = x;
}

static size_t *g_size_of, *g_first_of;
static int cmp_cluster(const void *a, const void *b) {
    const size_t x = *(const size_t *)a, y = *(const size_t *)b;
    if (g_size_of[x] != g_size_of[y]) return g_size_of[x] > g_size_of[y] ? -1 : 1;
    return g_first_of[x] < g_first_of[y] ? -1 : (g_first_of[x] > g_first_of[y]);
}

/* The serial Segment over nn lists (off / nb: CSR, entry (j, dist)). */
static void segment_lists(size_t n, const size_t *off, const size_t *nbj, const double *nbd, size_t min_size, size_t max_size,
                          size_t *offsets, size_t *indices, size_t *n_clusters, size_t *labels) {
    const size_t un = (size_t)-1;
    size_t *label = malloc(sizeof(size_t) * (n + 1)), *frontier = malloc(sizeof(size_t) * (n + 1));
    vec_t *merge = calloc(n + 1, sizeof(vec_t));
    for (size_t i = 0; i < n; ++i) label[i] = un;
    for (size_t i = 0; i < n; ++i) {
        if (label[i] != un) continue;
        push(&merge[i], i);
        size_t nf = 0;
        frontier[nf++] = i;
        label[i] = i;
        while (nf) {
            const size_t s = frontier[--nf];
            for (size_t k = off[s] + 1; k < off[s + 1]; ++k) {
                const size_t j = nbj[k];
                const size_t cl = label[j];
                if (cl == i || evaluate(s, j, nbd[k])) {
                    if (cl == un) {
                        frontier[nf++] = j;
                        label[j] = i;
                    } else if (cl != i) {
                        push(&merge[i], cl);
                    }
                }
            }
        }
    }
    /* symmetric */
    for (size_t i = 0; i < n; ++i) {
        const size_t m = merge[i].n;
        for (size_t k = 0; k < m; ++k) push(&merge[merge[i].v[k]], i);
    }
    /* closure: every point is a seed, so every label is an active seed */
    size_t *repr = malloc(sizeof(size_t) * (n + 1)), nc = 0;
    for (size_t i = 0; i < n; ++i) repr[i] = un;
    for (size_t i = 0; i < n; ++i) {
        if (label[i] != i || repr[i] != un) continue;   /* seed_active[i]: i labelled itself */
        size_t nf = 0;
        frontier[nf++] = i;
        repr[i] = nc;
        while (nf) {
            const size_t s = frontier[--nf];
            for (size_t k = 0; k < merge[s].n; ++k) {
                const size_t t = merge[s].v[k];
                if (repr[t] == un) {
                    frontier[nf++] = t;
                    repr[t] = nc;
                }
            }
        }
        ++nc;
    }
    /* segment_to_point_map_tmp with the `<= max` append */
    size_t *cnt = calloc(nc + 1, sizeof(size_t)), *first = malloc(sizeof(size_t) * (nc + 1));
    for (size_t c = 0; c < nc; ++c) first[c] = un;
    for (size_t i = 0; i < n; ++i) {
        const size_t c = repr[label[i]];
        if (cnt[c] <= max_size) {
            if (first[c] == un) first[c] = i;
            cnt[c]++;
        }
    }
    size_t *kept = malloc(sizeof(size_t) * (nc + 1)), nk = 0;
    for (size_t c = 0; c < nc; ++c)
        if (cnt[c] >= min_size && cnt[c] <= max_size) kept[nk++] = c;
    g_size_of = cnt;
    g_first_of = first;
    qsort(kept, nk, sizeof(size_t), cmp_cluster);
    size_t *rank = malloc(sizeof(size_t) * (nc + 1));
    for (size_t c = 0; c < nc; ++c) rank[c] = un;
    offsets[0] = 0;
    for (size_t k = 0; k < nk; ++k) {
        rank[kept[k]] = k;
        offsets[k + 1] = offsets[k] + cnt[kept[k]];
    }
    size_t *cur = malloc(sizeof(size_t) * (nk + 1));
    memcpy(cur, offsets, sizeof(size_t) * (nk + 1));
    for (size_t i = 0; i < n; ++i) {
        const size_t r = rank[repr[label[i]]];
        if (r != un) indices[cur[r]++] = i;
        labels[i] = r != un ? r : nk;
    }
    *n_clusters = nk;
    for (size_t i = 0; i < n; ++i) free(merge[i].v);
    free(merge); free(label); free(frontier); free(repr); free(cnt); free(first); free(kept); free(rank); free(cur);
}

static void set_eval(int kind, double dist, double angle_deg, const double *normals) {
    kind_g = kind;
    dist_g = dist;
    max_angle_g = angle_deg / 180 * M_PI;
    nrm_g = normals;
}

/* Segment(pc, radius, evaluator): KDTreeFlann radius lists (d2 <= r^2, self included) in (d2, index) order.  The
 * brute force runs over the points sorted by x: the scan from each point forwards stops once dx exceeds the radius
 * with a margin, and every pair is found from its first point in that order. */
static const double *g_xyz;
static int cmp_x(const void *a, const void *b) {
    const double x = g_xyz[3 * *(const size_t *)a], y = g_xyz[3 * *(const size_t *)b];
    return x < y ? -1 : (x > y);
}
void prox_ref_segment(const double *xyz, const double *normals, size_t n, double radius, int kind, double dist,
                      double angle_deg, size_t min_size, size_t max_size, size_t *offsets, size_t *indices,
                      size_t *n_clusters, size_t *labels) {
    set_eval(kind, dist, angle_deg, normals);
    const double r2 = radius * radius, reach = radius * 1.01 + 1e-300;
    size_t *ord = malloc(sizeof(size_t) * (n + 1)), nf = 0;
    for (size_t i = 0; i < n; ++i)
        if (isfinite(xyz[3 * i]) && isfinite(xyz[3 * i + 1]) && isfinite(xyz[3 * i + 2])) ord[nf++] = i;
    g_xyz = xyz;
    qsort(ord, nf, sizeof(size_t), cmp_x);
    vec_t *lists = calloc(n + 1, sizeof(vec_t));
    size_t total = 0;
    for (size_t a = 0; a < nf; ++a) {
        const size_t i = ord[a];
        for (size_t b = a; b < nf; ++b) {
            const size_t j = ord[b];
            if (xyz[3 * j] - xyz[3 * i] > reach) break;
            const double dx = xyz[3 * i] - xyz[3 * j], dy = xyz[3 * i + 1] - xyz[3 * j + 1], dz = xyz[3 * i + 2] - xyz[3 * j + 2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (!(d2 <= r2)) continue;
            push(&lists[i], j);
            total++;
            if (j != i) {
                push(&lists[j], i);
                total++;
            }
        }
    }
    size_t *off = malloc(sizeof(size_t) * (n + 1)), *nbj = malloc(sizeof(size_t) * (total + 1));
    double *nbd = malloc(sizeof(double) * (total + 1));
    nb_t *tmp = NULL;
    size_t tcap = 0;
    off[0] = 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t m = lists[i].n;
        if (m > tcap) {
            tcap = m;
            tmp = realloc(tmp, sizeof(nb_t) * tcap);
        }
        for (size_t k = 0; k < m; ++k) {
            const size_t j = lists[i].v[k];
            const double dx = xyz[3 * i] - xyz[3 * j], dy = xyz[3 * i + 1] - xyz[3 * j + 1], dz = xyz[3 * i + 2] - xyz[3 * j + 2];
            tmp[k].j = j;
            tmp[k].d2 = (dx * dx + dy * dy) + dz * dz;
        }
        qsort(tmp, m, sizeof(nb_t), cmp_nb);
        for (size_t k = 0; k < m; ++k) {
            nbj[off[i] + k] = tmp[k].j;
            nbd[off[i] + k] = sqrt(tmp[k].d2);
        }
        off[i + 1] = off[i] + m;
        free(lists[i].v);
    }
    segment_lists(n, off, nbj, nbd, min_size, max_size, offsets, indices, n_clusters, labels);
    free(lists); free(ord); free(off); free(nbj); free(nbd); free(tmp);
}

/* Segment(pc, nn_indices, evaluator): dist = (p_i - p_j).norm() */
void prox_ref_segment_nn(const double *xyz, const double *normals, size_t n, const size_t *nn_off, const size_t *nn_idx,
                         int kind, double dist, double angle_deg, size_t min_size, size_t max_size, size_t *offsets,
                         size_t *indices, size_t *n_clusters, size_t *labels) {
    set_eval(kind, dist, angle_deg, normals);
    const size_t total = nn_off[n];
    double *nbd = malloc(sizeof(double) * (total + 1));
    for (size_t i = 0; i < n; ++i)
        for (size_t k = nn_off[i]; k < nn_off[i + 1]; ++k) {
            const size_t j = nn_idx[k];
            const double dx = xyz[3 * i] - xyz[3 * j], dy = xyz[3 * i + 1] - xyz[3 * j + 1], dz = xyz[3 * i + 2] - xyz[3 * j + 2];
            nbd[k] = sqrt((dx * dx + dy * dy) + dz * dz);
        }
    segment_lists(n, nn_off, nn_idx, nbd, min_size, max_size, offsets, indices, n_clusters, labels);
    free(nbd);
}

/* the evaluators' threshold tests by themselves, vectorised for the cut-off check */
void prox_ref_dist_test(const double *d2, size_t m, double t, int distance_normals, uint8_t *out) {
    for (size_t k = 0; k < m; ++k) {
        const double dist = sqrt(d2[k]);
        out[k] = distance_normals ? !(dist >= t) : (dist < t);
    }
}
void prox_ref_angle_test(const double *dot, size_t m, double angle_deg, uint8_t *out) {
    const double max_angle = angle_deg / 180 * M_PI;
    for (size_t k = 0; k < m; ++k) {
        const double angle = acos(dot[k]);
        if (max_angle >= 0.0) {
            out[k] = angle <= max_angle;
        } else {
            const double b = M_PI - angle;
            out[k] = (b < angle ? b : angle) <= -max_angle;
        }
    }
}
