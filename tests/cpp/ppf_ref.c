/* ppf_ref.c -- the "PPF voting" and "PPF voting, EdgePoints mode" contracts of include/misc3d_amd.h in plain C, serial: the
 * table (rules M1 - M6, E1 - E5), the vote (V1 - V8, E6 - E8), the undefined places (U1 - U6) and K8's expected votes in
 * EdgePoints mode (E9).  The table pairs the sample with a referred set and the vote scans a cloud: in SampledPoints mode both
 * are the sample (the scene) itself, in EdgePoints mode the model's (the scene's) edge points.  Built by tests/ppf_ref_util.py
 * with -ffp-contract=off; with -fopenmp the two outer loops run in parallel (the cpu_baseline of tools/bench_configs.py) and
 * give the same output: every reference position has its own accumulator and its own list of maxima.  Nothing here is shared
 * with the library's sources. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct ppf_ref_model {
    size_t n;
    double r_min, angle_step, min_dist_thresh, min_angle_thresh;
    int angle_num, alpha_num, dist_num, k;
    size_t table_size, n_entries, n_neighbors;
    double *cos_edge, *alpha_c, *alpha_s, *dist_edge2;
    double centroid[3];
    double *pts, *nrm, *tmg;
    size_t n_e;          /* the referred set: the model's edge points as the table saw them; */
    double *epts, *enrm; /* NULL (and n_e == 0) in SampledPoints mode: the referred set is the sample */
    uint32_t *cell_off, *nbr_off, *nbr_idx;
    uint16_t* entry_i;
    uint8_t* entry_alpha;
} ppf_ref_model;

/* rule M3 */
void ppf_ref_frame(const double* p, const double* n, double* T) {
    double u1 = n[2], u2 = -n[1];
    const double norm = sqrt(u1 * u1 + u2 * u2);
    if (norm > 1.0e-6) {
        const double inv = 1 / norm;
        u1 *= inv;
        u2 *= inv;
    } else {
        u1 = 1.0;
        u2 = 0.0;
    }
    double nx = n[0];
    if (nx > 1.0) nx = 1.0;
    if (nx < -1.0) nx = -1.0;
    const double half = acos(nx) / 2;
    const double q[4] = {cos(half), 0.0, sin(half) * u1, sin(half) * u2};
    double R[3][3];
    R[0][0] = 1 - 2 * (q[2] * q[2] + q[3] * q[3]);
    R[0][1] = 2 * (q[1] * q[2] - q[0] * q[3]);
    R[0][2] = 2 * (q[0] * q[2] + q[1] * q[3]);
    R[1][0] = 2 * (q[1] * q[2] + q[0] * q[3]);
    R[1][1] = 1 - 2 * (q[1] * q[1] + q[3] * q[3]);
    R[1][2] = 2 * (q[2] * q[3] - q[0] * q[1]);
    R[2][0] = 2 * (q[1] * q[3] - q[0] * q[2]);
    R[2][1] = 2 * (q[0] * q[1] + q[2] * q[3]);
    R[2][2] = 1 - 2 * (q[1] * q[1] + q[2] * q[2]);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[4 * r + c] = R[r][c];
        T[4 * r + 3] = -((R[r][0] * p[0] + R[r][1] * p[1]) + R[r][2] * p[2]);
    }
    T[12] = T[13] = T[14] = 0.0;
    T[15] = 1.0;
}

static int angle_bin(const ppf_ref_model* M, double x) {
    int b = 0;
    for (int k = 0; k < M->angle_num - 1; ++k)
        if (x <= M->cos_edge[k]) ++b;
    return b;
}

static int alpha_bin(const ppf_ref_model* M, double y, double z) {
    const double v = -z;
    if (y == 0.0 && v == 0.0) return M->angle_num - 1;
    const int upper = !signbit(v);
    int b = 0;
    for (int k = 0; k < M->alpha_num - 1; ++k) {
        const int ccw = M->alpha_c[k] * v - M->alpha_s[k] * y >= 0.0;
        if (M->alpha_s[k] > 0.0 ? (upper && ccw) : (upper || ccw)) ++b;
    }
    return b;
}

/* rule M4 with U2 - U4: 1 and q[0..3], *qa, or 0 for a pair that is skipped; T = the 4 x 4 frame of p0 */
int ppf_ref_pair_bins(const ppf_ref_model* M, const double* p0, const double* n0, const double* p1, const double* n1, const double* T,
                      int* q, int* qa) {
    const double dx = p1[0] - p0[0], dy = p1[1] - p0[1], dz = p1[2] - p0[2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (!(d2 > 0.0)) return 0;
    int qd = 0;
    for (int k = 0; k < M->dist_num; ++k)
        if (d2 >= M->dist_edge2[k]) ++qd;
    if (qd >= M->dist_num) return 0;
    const double norm = sqrt(d2);
    const double ux = dx / norm, uy = dy / norm, uz = dz / norm;
    q[0] = angle_bin(M, (n0[0] * ux + n0[1] * uy) + n0[2] * uz);
    q[1] = angle_bin(M, (n1[0] * ux + n1[1] * uy) + n1[2] * uz);
    q[2] = angle_bin(M, (n0[0] * n1[0] + n0[1] * n1[1]) + n0[2] * n1[2]);
    q[3] = qd;
    const double y = ((T[4] * p1[0] + T[5] * p1[1]) + T[6] * p1[2]) + T[7];
    const double z = ((T[8] * p1[0] + T[9] * p1[1]) + T[10] * p1[2]) + T[11];
    *qa = alpha_bin(M, y, z);
    return 1;
}

/* SpreadPPF: the loop nest of ppf_estimation.cpp:719-742 -> the number of cells */
int ppf_ref_spread(const ppf_ref_model* M, const int* q, int64_t* cells) {
    int n = 0;
    const int64_t a = M->angle_num;
    for (int s0 = 0; s0 < 3; ++s0) {
        const int d = q[3] + s0 - 1;
        if (d < 0 || d >= M->dist_num) continue;
        for (int s1 = 0; s1 < M->k; ++s1) {
            const int a0 = q[0] + s1 - 1;
            if (a0 < 0 || a0 >= M->angle_num) continue;
            for (int s2 = 0; s2 < M->k; ++s2) {
                const int a1 = q[1] + s2 - 1;
                if (a1 < 0 || a1 >= M->angle_num) continue;
                for (int s3 = 0; s3 < M->k; ++s3) {
                    const int a2 = q[2] + s3 - 1;
                    if (a2 < 0 || a2 >= M->angle_num) continue;
                    cells[n++] = a0 + a * (a1 + a * (a2 + a * d));
                }
            }
        }
    }
    return n;
}

void ppf_ref_destroy(ppf_ref_model* M) {
    if (!M) return;
    free(M->cos_edge);
    free(M->alpha_c);
    free(M->alpha_s);
    free(M->dist_edge2);
    free(M->pts);
    free(M->nrm);
    free(M->tmg);
    free(M->epts);
    free(M->enrm);
    free(M->cell_off);
    free(M->nbr_off);
    free(M->nbr_idx);
    free(M->entry_i);
    free(M->entry_alpha);
    free(M);
}

/* M1 - M6, or E1 - E5 when edge_points / edge_normals (n_e of them) are given: NULL means SampledPoints.  centre_edges == 0
 * leaves the edge set uncentred, as the reference does (ppf_estimation.cpp:588-589): the variant tests/test_ppf_edge.py uses
 * to show why E1 deviates; every other caller passes 1.  n may be 0: the sizes and edge tables alone (no points, no table),
 * which the hand cases use. */
ppf_ref_model* ppf_ref_create(const double* points, const double* normals, size_t n, const double* edge_points,
                              const double* edge_normals, size_t n_e, double diameter, double r_min, double rel_sample_dist,
                              double angle_step, double min_dist_thresh, double min_angle_thresh, int faster_mode,
                              int centre_edges) {
    ppf_ref_model* M = (ppf_ref_model*)calloc(1, sizeof(ppf_ref_model));
    M->n = n;
    M->r_min = r_min;
    M->angle_step = angle_step;
    M->min_dist_thresh = min_dist_thresh;
    M->min_angle_thresh = min_angle_thresh;
    M->angle_num = (int)(round(M_PI / angle_step) + 1.0);
    M->alpha_num = 2 * M->angle_num - 1;
    M->dist_num = (int)(round(1.0 / rel_sample_dist) + 1.0);
    M->k = faster_mode ? 2 : 3;
    M->table_size = (size_t)M->angle_num * M->angle_num * M->angle_num * M->dist_num;
    const double dist_step = diameter * rel_sample_dist;
    M->cos_edge = (double*)calloc(M->angle_num, sizeof(double));
    M->alpha_c = (double*)calloc(M->alpha_num, sizeof(double));
    M->alpha_s = (double*)calloc(M->alpha_num, sizeof(double));
    M->dist_edge2 = (double*)calloc(M->dist_num, sizeof(double));
    for (int k = 0; k < M->angle_num - 1; ++k) M->cos_edge[k] = cos(((double)k + 0.5) * angle_step);
    for (int b = 0; b < M->alpha_num - 1; ++b) {
        const double th = ((double)b + 0.5) * angle_step - M_PI;
        M->alpha_c[b] = th <= M_PI ? cos(th) : NAN;   /* an edge beyond pi is never passed */
        M->alpha_s[b] = th <= M_PI ? sin(th) : 1.0;
    }
    for (int k = 0; k < M->dist_num; ++k) {
        const double e = ((double)k + 0.5) * dist_step;
        M->dist_edge2[k] = e * e;
    }
    if (n == 0) return M;
    /* M2, M3 */
    M->pts = (double*)malloc(sizeof(double) * 3 * n);
    M->nrm = (double*)malloc(sizeof(double) * 3 * n);
    M->tmg = (double*)malloc(sizeof(double) * 16 * n);
    double c[3] = {0, 0, 0};
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) c[k] += points[3 * i + k];
    for (int k = 0; k < 3; ++k) M->centroid[k] = c[k] / (double)n;
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) {
            M->pts[3 * i + k] = points[3 * i + k] - M->centroid[k];
            M->nrm[3 * i + k] = normals[3 * i + k];
        }
        ppf_ref_frame(M->pts + 3 * i, M->nrm + 3 * i, M->tmg + 16 * i);
    }
    /* E1: the edge set is centred by the centroid of the sample alone */
    const int same = edge_points == NULL;
    if (!same) {
        M->n_e = n_e;
        M->epts = (double*)malloc(sizeof(double) * 3 * n_e);
        M->enrm = (double*)malloc(sizeof(double) * 3 * n_e);
        for (size_t j = 0; j < n_e; ++j)
            for (int k = 0; k < 3; ++k) {
                M->epts[3 * j + k] = centre_edges ? edge_points[3 * j + k] - M->centroid[k] : edge_points[3 * j + k];
                M->enrm[3 * j + k] = edge_normals[3 * j + k];
            }
    }
    const double *rp = same ? M->pts : M->epts, *rn = same ? M->nrm : M->enrm;   /* the referred set, n_r points */
    const size_t n_r = same ? n : n_e, pairs = n * n_r;
    /* M4, M5 / E3, E4: keys of all ordered pairs (i in the sample, j in the referred set; i == j is left out only when the two
     * are the same set), then a counting sort in (i, j) order */
    const size_t H = M->table_size;
    uint32_t* cell = (uint32_t*)malloc(sizeof(uint32_t) * pairs);
    uint8_t* qal = (uint8_t*)malloc(pairs);
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)n; ++i)
        for (size_t j = 0; j < n_r; ++j) {
            int q[4], qa = 0;
            uint32_t key = (uint32_t)H;
            if (!(same && (size_t)i == j) && ppf_ref_pair_bins(M, M->pts + 3 * i, M->nrm + 3 * i, rp + 3 * j, rn + 3 * j, M->tmg + 16 * i, q, &qa))
                key = (uint32_t)(q[0] + M->angle_num * (q[1] + M->angle_num * (q[2] + (size_t)M->angle_num * q[3])));
            cell[(size_t)i * n_r + j] = key;
            qal[(size_t)i * n_r + j] = (uint8_t)qa;
        }
    M->cell_off = (uint32_t*)calloc(H + 2, sizeof(uint32_t));
    for (size_t p = 0; p < pairs; ++p) ++M->cell_off[cell[p] + 1];
    for (size_t c2 = 0; c2 <= H; ++c2) M->cell_off[c2 + 1] += M->cell_off[c2];
    M->n_entries = M->cell_off[H];
    M->entry_i = (uint16_t*)malloc(sizeof(uint16_t) * (M->n_entries + 1));
    M->entry_alpha = (uint8_t*)malloc(M->n_entries + 1);
    uint32_t* fill = (uint32_t*)malloc(sizeof(uint32_t) * (H + 1));
    memcpy(fill, M->cell_off, sizeof(uint32_t) * (H + 1));
    for (size_t p = 0; p < pairs; ++p) {
        if (cell[p] >= H) continue;
        const uint32_t at = fill[cell[p]]++;
        M->entry_i[at] = (uint16_t)(p / n_r);
        M->entry_alpha[at] = qal[p];
    }
    free(fill);
    free(cell);
    free(qal);
    /* M6 = E5, over the sample */
    const double r = 0.5 * r_min, r2 = r * r;
    M->nbr_off = (uint32_t*)calloc(n + 1, sizeof(uint32_t));
    for (int pass = 0; pass < 2; ++pass) {
        size_t at = 0;
        for (size_t i = 0; i < n; ++i) {
            if (pass == 0) M->nbr_off[i] = (uint32_t)at;
            for (size_t j = 0; j < n; ++j) {
                const double dx = M->pts[3 * j] - M->pts[3 * i], dy = M->pts[3 * j + 1] - M->pts[3 * i + 1],
                             dz = M->pts[3 * j + 2] - M->pts[3 * i + 2];
                if ((dx * dx + dy * dy) + dz * dz < r2) {
                    if (pass == 1) M->nbr_idx[at] = (uint32_t)j;
                    ++at;
                }
            }
        }
        if (pass == 0) {
            M->nbr_off[n] = (uint32_t)at;
            M->n_neighbors = at;
            M->nbr_idx = (uint32_t*)malloc(sizeof(uint32_t) * (at + 1));
        }
    }
    return M;
}

void ppf_ref_sizes(const ppf_ref_model* M, uint64_t* out) {
    out[0] = M->table_size;
    out[1] = M->n_entries;
    out[2] = M->n_neighbors;
    out[3] = (uint64_t)M->angle_num;
    out[4] = (uint64_t)M->alpha_num;
    out[5] = (uint64_t)M->dist_num;
}

void ppf_ref_table(const ppf_ref_model* M, uint32_t* cell_off, uint16_t* entry_i, uint8_t* entry_alpha, uint32_t* nbr_off,
                   uint32_t* nbr_idx, double* tmg, double* centroid) {
    if (cell_off) memcpy(cell_off, M->cell_off, sizeof(uint32_t) * (M->table_size + 1));
    if (entry_i) memcpy(entry_i, M->entry_i, sizeof(uint16_t) * M->n_entries);
    if (entry_alpha) memcpy(entry_alpha, M->entry_alpha, M->n_entries);
    if (nbr_off) memcpy(nbr_off, M->nbr_off, sizeof(uint32_t) * (M->n + 1));
    if (nbr_idx) memcpy(nbr_idx, M->nbr_idx, sizeof(uint32_t) * M->n_neighbors);
    if (tmg) memcpy(tmg, M->tmg, sizeof(double) * 16 * M->n);
    if (centroid) memcpy(centroid, M->centroid, sizeof(double) * 3);
}

/* CalcLocalMaximum (ppf_estimation.cpp:1170-1234), rule V7: out = triples (row, column, votes) -> their number */
size_t ppf_ref_local_maximum(const uint32_t* acc, size_t rows, size_t cols, size_t vote_threshold, const uint32_t* nbr_off,
                             const uint32_t* nbr_idx, uint32_t* out) {
    uint32_t* best = (uint32_t*)malloc(sizeof(uint32_t) * rows);
    uint32_t* col = (uint32_t*)malloc(sizeof(uint32_t) * rows);
    const size_t last = cols - 1;
    size_t max_votes = 0, found = 0;
    for (size_t r = 0; r < rows; ++r) {
        const uint32_t* a = acc + r * cols;
        best[r] = a[cols - 1] + a[0] + a[1];
        col[r] = 0;
        for (size_t c = 1; c < last; ++c) {
            const uint32_t t = a[c - 1] + a[c] + a[c + 1];
            if (t > best[r]) {
                best[r] = t;
                col[r] = (uint32_t)c;
            }
        }
        const uint32_t t = a[last - 1] + a[last] + a[0];
        if (t > best[r]) {
            best[r] = t;
            col[r] = (uint32_t)last;
        }
        if (best[r] > max_votes) max_votes = best[r];
    }
    if (max_votes >= vote_threshold) {
        const size_t thr = (size_t)((double)max_votes * 0.8);
        unsigned char* flag = (unsigned char*)malloc(rows);
        memset(flag, 1, rows);
        for (size_t i = 0; i < rows; ++i) {
            if (!(best[i] > thr && flag[i])) continue;
            int is_max = 1;
            for (uint32_t t = nbr_off[i]; t < nbr_off[i + 1]; ++t) {
                const uint32_t j = nbr_idx[t];
                if (best[i] < best[j])
                    is_max = 0;
                else
                    flag[j] = 0;
            }
            flag[i] = (unsigned char)is_max;
            if (is_max) {
                out[3 * found] = (uint32_t)i;
                out[3 * found + 1] = col[i];
                out[3 * found + 2] = best[i];
                ++found;
            }
        }
        free(flag);
    }
    free(best);
    free(col);
    return found;
}

static void mul4(const double* A, const double* B, double* C) {
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            C[4 * r + c] = ((A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c]) + A[4 * r + 3] * B[12 + c];
}

/* rule V8: tsg^-1 Rx(alpha) tmg, the inverse being [R^T | -R^T t] */
static void pose_product(const double* tsg, double alpha, const double* tmg, double* out) {
    double inv[16], tmp[16];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) inv[4 * r + c] = tsg[4 * c + r];
        inv[4 * r + 3] = -((tsg[r] * tsg[3] + tsg[4 + r] * tsg[7]) + tsg[8 + r] * tsg[11]);
    }
    inv[12] = inv[13] = inv[14] = 0.0;
    inv[15] = 1.0;
    const double ca = cos(alpha), sa = sin(alpha);
    const double rx[16] = {1, 0, 0, 0, 0, ca, -sa, 0, 0, sa, ca, 0, 0, 0, 0, 1};
    mul4(inv, rx, tmp);
    mul4(tmp, tmg, out);
}

/* V1 - V8, or E6 - E8 when the scene's edge points ep / en (m_e of them) are given: NULL means SampledPoints.  The reference
 * points are read from the scene sample sp / sn (m points); the neighbours are searched in the scanned cloud: the sample itself,
 * or the edge points.  The result arrays hold cap entries each (poses cap x 16, may be NULL); n_searched (may be NULL): n_ref
 * counts; stats[0] += neighbours visited, stats[1] += increments.  Returns the number of maxima (nothing is written past cap). */
size_t ppf_ref_vote(const ppf_ref_model* M, const double* sp, const double* sn, size_t m, const size_t* reference, size_t n_ref,
                    const double* ep, const double* en, size_t m_e, size_t cap, uint32_t* ref_pos, uint32_t* model_index,
                    uint32_t* alpha_index, uint32_t* votes, double* poses, uint32_t* n_searched, uint64_t* stats) {
    const size_t n = M->n, A = (size_t)M->alpha_num, H = M->table_size;
    const size_t gate = (size_t)((double)(M->epts ? M->n_e : n) * 0.2);   /* V3 / E7: refered_model_num */
    const double *cp = ep ? ep : sp, *cn = ep ? en : sn;                  /* the scanned cloud, m_c points */
    const size_t m_c = ep ? m_e : m;
    const double r2 = M->r_min * M->r_min, dist_thresh = M->min_dist_thresh * M->r_min, cos_thresh = cos(M->min_angle_thresh);
    uint32_t** found = (uint32_t**)calloc(n_ref, sizeof(uint32_t*));
    size_t* n_found = (size_t*)calloc(n_ref, sizeof(size_t));
    uint64_t visited = 0, increments = 0;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : visited, increments)
    for (long long s = 0; s < (long long)n_ref; ++s) {
        const double* p0 = sp + 3 * reference[s];
        const double* n0 = sn + 3 * reference[s];
        double tsg[16];
        ppf_ref_frame(p0, n0, tsg);
        size_t searched = 0;
        for (size_t j = 0; j < m_c; ++j) {
            const double dx = cp[3 * j] - p0[0], dy = cp[3 * j + 1] - p0[1], dz = cp[3 * j + 2] - p0[2];
            if ((dx * dx + dy * dy) + dz * dz < r2) ++searched;
        }
        if (n_searched) n_searched[s] = (uint32_t)searched;
        visited += searched;
        if (!(searched > gate)) continue;
        uint32_t* acc = (uint32_t*)calloc(n * A, sizeof(uint32_t));
        uint64_t* flags = (uint64_t*)calloc(H, sizeof(uint64_t));
        for (size_t j = 0; j < m_c; ++j) {
            const double* p1 = cp + 3 * j;
            const double* n1 = cn + 3 * j;
            const double dx = p1[0] - p0[0], dy = p1[1] - p0[1], dz = p1[2] - p0[2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (!(d2 < r2)) continue;
            if (sqrt(d2) < dist_thresh && (n1[0] * n0[0] + n1[1] * n0[1]) + n1[2] * n0[2] > cos_thresh) continue;
            int q[4], qa;
            if (!ppf_ref_pair_bins(M, p0, n0, p1, n1, tsg, q, &qa)) continue;
            int64_t cells[81];
            const int nc = ppf_ref_spread(M, q, cells);
            for (int c = 0; c < nc; ++c) {
                const uint64_t bit = (uint64_t)1 << qa;
                if (flags[cells[c]] & bit) continue;
                flags[cells[c]] |= bit;
                for (uint32_t t = M->cell_off[cells[c]]; t < M->cell_off[cells[c] + 1]; ++t) {
                    ++acc[(size_t)M->entry_i[t] * A + (size_t)(((int)M->entry_alpha[t] - qa + (int)A) % (int)A)];
                    ++increments;
                }
            }
        }
        found[s] = (uint32_t*)malloc(sizeof(uint32_t) * 3 * n);
        n_found[s] = ppf_ref_local_maximum(acc, n, A, gate, M->nbr_off, M->nbr_idx, found[s]);
        free(acc);
        free(flags);
    }
    size_t total = 0;
    for (size_t s = 0; s < n_ref; ++s) {
        for (size_t k = 0; k < n_found[s]; ++k, ++total) {
            if (total >= cap) continue;
            const uint32_t* f = found[s] + 3 * k;
            ref_pos[total] = (uint32_t)s;
            model_index[total] = f[0];
            alpha_index[total] = f[1];
            votes[total] = f[2];
            if (poses) {
                double tsg[16];
                ppf_ref_frame(sp + 3 * reference[s], sn + 3 * reference[s], tsg);
                pose_product(tsg, (double)f[1] * M->angle_step, M->tmg + 16 * (size_t)f[0], poses + 16 * total);
            }
        }
        free(found[s]);
    }
    free(found);
    free(n_found);
    if (stats) {
        stats[0] += visited;
        stats[1] += increments;
    }
    return total;
}

/* E9: K8's score in EdgePoints mode, expected = (ratio n) n without the 0.25; votes sorted descending.  scores (k) are filled;
 * -> the number of results kept by score_thresh and num_result. */
size_t ppf_ref_edge_scores(const uint64_t* votes, size_t k, double ratio, uint64_t n_model, double score_thresh, int num_result,
                           double* scores) {
    const double expected = (ratio * (double)n_model) * (double)n_model;
    size_t keep = k;
    for (size_t i = 0; i < k; ++i) {
        const double s = (double)votes[i] / expected;
        scores[i] = s < 1.0 ? s : 1.0;
    }
    for (size_t i = 0; i < k; ++i)
        if (scores[i] < score_thresh) {
            keep = i;
            break;
        }
    if (num_result >= 0 && keep > (size_t)num_result) keep = (size_t)num_result;
    return keep;
}
