/* fpfh_ref.c -- plain-C brute-force restatement of the "fragment preprocessing" contract of include/misc3d_amd.h
 * (neighbourhood, normals, FPFH), written from the contract's text.  Built by tests/fpfh_ref_util.py at test time
 * (-ffp-contract=off; -fopenmp only spreads the independent per-point loops over threads). */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MAXNN 128

static int finite3(const double *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

/* the list of point i: up to max_nn nearest by (d2, index), d2 finite, d2 < r2 for Hybrid; returns m */
static int neighbours(const double *xyz, size_t n, size_t i, int hybrid, double r2, int max_nn, int64_t *idx, double *dd) {
    int m = 0;
    const double *q = xyz + 3 * i;
    if (!finite3(q)) return 0;
    for (size_t j = 0; j < n; ++j) {
        const double *p = xyz + 3 * j;
        const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (!isfinite(d2)) continue;
        if (hybrid && !(d2 < r2)) continue;
        if (m == max_nn && !(d2 < dd[m - 1])) continue;   /* j ascends: an equal d2 with a larger index loses */
        int k = m < max_nn ? m++ : max_nn - 1;
        while (k > 0 && d2 < dd[k - 1]) {
            dd[k] = dd[k - 1];
            idx[k] = idx[k - 1];
            --k;
        }
        dd[k] = d2;
        idx[k] = (int64_t)j;
    }
    return m;
}

void fpfh_ref_neighbours(const double *xyz, size_t n, int search, double radius, int max_nn, int64_t *idx, double *d2,
                         int32_t *cnt) {
    const double r2 = radius * radius;
#pragma omp parallel for schedule(dynamic, 64)
    for (size_t i = 0; i < n; ++i) {
        int64_t li[MAXNN];
        double ld[MAXNN];
        const int m = neighbours(xyz, n, i, search == 2, r2, max_nn, li, ld);
        cnt[i] = m;
        for (int k = 0; k < max_nn; ++k) {
            idx[i * (size_t)max_nn + k] = k < m ? li[k] : -1;
            d2[i * (size_t)max_nn + k] = k < m ? ld[k] : INFINITY;
        }
    }
}

static double dot(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

static void pair_features(const double *p1, const double *n1, const double *p2, const double *n2, double *f) {
    double dp[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    f[0] = f[1] = f[2] = 0.0;
    const double d = sqrt(dot(dp, dp));
    if (d == 0.0) return;
    const double a1 = dot(n1, dp) / d, a2 = dot(n2, dp) / d;
    const double *na = n1, *nb = n2;
    double f2;
    if (acos(fabs(a1)) > acos(fabs(a2))) {
        na = n2;
        nb = n1;
        dp[0] = -dp[0];
        dp[1] = -dp[1];
        dp[2] = -dp[2];
        f2 = -a2;
    } else {
        f2 = a1;
    }
    double v[3] = {dp[1] * na[2] - dp[2] * na[1], dp[2] * na[0] - dp[0] * na[2], dp[0] * na[1] - dp[1] * na[0]};
    const double vn = sqrt(dot(v, v));
    if (vn == 0.0) return;
    v[0] /= vn;
    v[1] /= vn;
    v[2] /= vn;
    const double w[3] = {na[1] * v[2] - na[2] * v[1], na[2] * v[0] - na[0] * v[2], na[0] * v[1] - na[1] * v[0]};
    f[2] = f2;
    f[1] = dot(v, nb);
    f[0] = atan2(dot(w, nb), dot(na, nb));
}

static int clamp_bin(double x) {
    const double h = floor(x);
    if (!(h >= 0.0)) return 0;
    if (h > 10.0) return 10;
    return (int)h;
}
static void bins_of(const double *f, int *b) {
    b[0] = clamp_bin(11.0 * (f[0] + M_PI) / (2.0 * M_PI));
    b[1] = 11 + clamp_bin(11.0 * (f[1] + 1.0) * 0.5);
    b[2] = 22 + clamp_bin(11.0 * (f[2] + 1.0) * 0.5);
}

void fpfh_ref_pair_bins(const double *pairs, size_t m, int32_t *bins, double *feat) {
    for (size_t t = 0; t < m; ++t) {
        const double *p = pairs + 12 * t;
        double f[3];
        int b[3];
        pair_features(p, p + 3, p + 6, p + 9, f);
        bins_of(f, b);
        for (int k = 0; k < 3; ++k) {
            bins[3 * t + k] = b[k];
            if (feat) feat[3 * t + k] = f[k];
        }
    }
}

/* out: n x 33; spfh_out (may be NULL): n x 33 */
void fpfh_ref_compute(const double *xyz, const double *normals, size_t n, int search, double radius, int max_nn, double *out,
                      double *spfh_out) {
    const double r2 = radius * radius;
    double *spfh = (double *)calloc(n * 33 + 1, sizeof(double));
    int64_t *idx = (int64_t *)malloc(sizeof(int64_t) * (n * (size_t)max_nn + 1));
    double *dd = (double *)malloc(sizeof(double) * (n * (size_t)max_nn + 1));
    int32_t *cnt = (int32_t *)malloc(sizeof(int32_t) * (n + 1));
#pragma omp parallel for schedule(dynamic, 64)
    for (size_t i = 0; i < n; ++i) {
        int64_t *li = idx + i * (size_t)max_nn;
        double *ld = dd + i * (size_t)max_nn;
        const int m = neighbours(xyz, n, i, search == 2, r2, max_nn, li, ld);
        cnt[i] = m;
        if (m <= 1) continue;
        const double incr = 100.0 / (double)(m - 1);
        for (int k = 1; k < m; ++k) {
            double f[3];
            int b[3];
            pair_features(xyz + 3 * i, normals + 3 * i, xyz + 3 * li[k], normals + 3 * li[k], f);
            bins_of(f, b);
            for (int t = 0; t < 3; ++t) spfh[i * 33 + b[t]] += incr;
        }
    }
#pragma omp parallel for schedule(dynamic, 64)
    for (size_t i = 0; i < n; ++i) {
        double *o = out + i * 33;
        for (int j = 0; j < 33; ++j) o[j] = 0.0;
        const int m = cnt[i];
        if (m <= 1) continue;
        const int64_t *li = idx + i * (size_t)max_nn;
        const double *ld = dd + i * (size_t)max_nn;
        double acc[33], sum[3] = {0.0, 0.0, 0.0};
        for (int j = 0; j < 33; ++j) acc[j] = 0.0;
        for (int k = 1; k < m; ++k) {
            if (ld[k] == 0.0) continue;
            for (int j = 0; j < 33; ++j) {
                const double val = spfh[li[k] * 33 + j] / ld[k];
                acc[j] += val;
                sum[j / 11] += val;
            }
        }
        for (int g = 0; g < 3; ++g)
            if (sum[g] != 0.0) sum[g] = 100.0 / sum[g];
        for (int j = 0; j < 33; ++j) o[j] = acc[j] * sum[j / 11] + spfh[i * 33 + j];
    }
    if (spfh_out) memcpy(spfh_out, spfh, sizeof(double) * n * 33);
    free(spfh);
    free(idx);
    free(dd);
    free(cnt);
}

/* cyclic Jacobi on a symmetric 3 x 3; the unit eigenvector of the smallest eigenvalue */
static void smallest_eigvec(const double *Cin, double *nrm) {
    double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) A[r][c] = Cin[3 * r + c];
    for (int sweep = 0; sweep < 24; ++sweep) {
        if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[1][2] == 0.0) break;
        for (int e = 0; e < 3; ++e) {
            const int p = e == 2 ? 1 : 0, q = e == 0 ? 1 : 2;
            if (A[p][q] == 0.0) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            for (int k = 0; k < 3; ++k) {
                const double akp = A[k][p], akq = A[k][q];
                A[k][p] = c * akp - s * akq;
                A[k][q] = s * akp + c * akq;
            }
            for (int k = 0; k < 3; ++k) {
                const double apk = A[p][k], aqk = A[q][k];
                A[p][k] = c * apk - s * aqk;
                A[q][k] = s * apk + c * aqk;
            }
            A[p][q] = A[q][p] = 0.0;
            for (int k = 0; k < 3; ++k) {
                const double vkp = V[k][p], vkq = V[k][q];
                V[k][p] = c * vkp - s * vkq;
                V[k][q] = s * vkp + c * vkq;
            }
        }
    }
    int m = 0;
    if (A[1][1] < A[m][m]) m = 1;
    if (A[2][2] < A[m][m]) m = 2;
    const double l = sqrt((V[0][m] * V[0][m] + V[1][m] * V[1][m]) + V[2][m] * V[2][m]);
    nrm[0] = V[0][m] / l;
    nrm[1] = V[1][m] / l;
    nrm[2] = V[2][m] / l;
}

void fpfh_ref_normals(const double *xyz, size_t n, int search, double radius, int max_nn, int orient, const double *cam,
                      double *out) {
    const double r2 = radius * radius;
#pragma omp parallel for schedule(dynamic, 64)
    for (size_t i = 0; i < n; ++i) {
        int64_t li[MAXNN];
        double ld[MAXNN];
        const int m = neighbours(xyz, n, i, search == 2, r2, max_nn, li, ld);
        double nn[3] = {0.0, 0.0, 1.0};
        if (m >= 3) {
            double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int k = 0; k < m; ++k) {
                const double *p = xyz + 3 * li[k];
                s[0] += p[0];
                s[1] += p[1];
                s[2] += p[2];
                s[3] += p[0] * p[0];
                s[4] += p[0] * p[1];
                s[5] += p[0] * p[2];
                s[6] += p[1] * p[1];
                s[7] += p[1] * p[2];
                s[8] += p[2] * p[2];
            }
            for (int t = 0; t < 9; ++t) s[t] *= 1.0 / (double)m;
            const double C[9] = {s[3] - s[0] * s[0], s[4] - s[0] * s[1], s[5] - s[0] * s[2],
                                 s[4] - s[0] * s[1], s[6] - s[1] * s[1], s[7] - s[1] * s[2],
                                 s[5] - s[0] * s[2], s[7] - s[1] * s[2], s[8] - s[2] * s[2]};
            smallest_eigvec(C, nn);
            if (!(dot(nn, nn) > 0.0)) {
                nn[0] = nn[1] = 0.0;
                nn[2] = 1.0;
            }
        }
        if (orient) {
            const double *p = xyz + 3 * i;
            const double v[3] = {cam[0] - p[0], cam[1] - p[1], cam[2] - p[2]};
            if (nn[0] == 0.0 && nn[1] == 0.0 && nn[2] == 0.0) {
                const double l = sqrt(dot(v, v));
                if (l == 0.0) {
                    nn[2] = 1.0;
                } else {
                    nn[0] = v[0] / l;
                    nn[1] = v[1] / l;
                    nn[2] = v[2] / l;
                }
            } else if (dot(nn, v) < 0.0) {
                nn[0] = -nn[0];
                nn[1] = -nn[1];
                nn[2] = -nn[2];
            }
        }
        memcpy(out + 3 * i, nn, sizeof(nn));
    }
}
