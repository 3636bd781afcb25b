/* icp_ref.c -- a plain-C, one-thread restatement of the ICP contract of include/misc3d_amd.h (m3d_registration_icp,
 * m3d_registration_icp_plane): Open3D 0.15.1 RegistrationICP with TransformationEstimationPointToPoint or
 * TransformationEstimationPointToPlane, restated from the numbered rules there.  The checker of the GPU tests; built by
 * tests/icp_ref_util.py with gcc -O2 -ffp-contract=off.  Nothing here is shared with the library:
 *   - the search is a uniform grid of its own (cells of the search radius, 27 cells per query), lowest target index on
 *     exact ties of the squared distance (dx dx + dy dy) + dz dz;
 *   - every sum runs serially over the source index, ascending (order >= 0) or descending (order < 0: the input guard of
 *     the tests compares the two);
 *   - point-to-plane: its own 6 x 6 elimination for the determinant, an unpivoted LDL^T for the solve, the rotation as the
 *     product of three matrices;
 *   - point-to-point: the rotation by Horn's quaternion method (Jacobi on the 4 x 4 matrix), not an SVD.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    double lo[3], h, r2;
    int64_t n[3];
    uint32_t *start, *idx; /* cells' first slots (ncell + 1), target indices sorted by cell, ascending inside a cell */
    const double *pts;
    int empty;
} Grid;

static int finite3(const double *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

static int cell_of(const Grid *g, const double *p, int64_t c[3]) {
    for (int k = 0; k < 3; ++k) {
        const double f = floor((p[k] - g->lo[k]) / g->h);
        if (!(f >= 0.0 && f < (double)g->n[k])) return 0;
        c[k] = (int64_t)f;
    }
    return 1;
}

static int grid_build(Grid *g, const double *dst, size_t nd, double radius) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    memset(g, 0, sizeof(*g));
    g->pts = dst;
    g->r2 = radius * radius;
    for (size_t j = 0; j < nd; ++j)
        if (finite3(dst + 3 * j))
            for (int k = 0; k < 3; ++k) {
                if (dst[3 * j + k] < lo[k]) lo[k] = dst[3 * j + k];
                if (dst[3 * j + k] > hi[k]) hi[k] = dst[3 * j + k];
            }
    if (!(lo[0] <= hi[0])) {
        g->empty = 1;
        return 0;
    }
    double h = radius;
    for (;;) { /* at most 2^24 cells: a larger cell still holds every neighbour within the radius in the 27 cells */
        double total = 1.0;
        for (int k = 0; k < 3; ++k) {
            g->lo[k] = lo[k] - h;
            g->n[k] = (int64_t)floor((hi[k] - g->lo[k]) / h) + 2;
            total *= (double)g->n[k];
        }
        if (total <= 16777216.0) break;
        h *= 2.0;
    }
    g->h = h;
    const size_t ncell = (size_t)(g->n[0] * g->n[1] * g->n[2]);
    g->start = (uint32_t *)calloc(ncell + 1, sizeof(uint32_t));
    g->idx = (uint32_t *)malloc(sizeof(uint32_t) * (nd ? nd : 1));
    if (!g->start || !g->idx) return -1;
    int64_t c[3];
    for (size_t j = 0; j < nd; ++j)
        if (finite3(dst + 3 * j) && cell_of(g, dst + 3 * j, c)) g->start[(c[2] * g->n[1] + c[1]) * g->n[0] + c[0] + 1]++;
    for (size_t k = 0; k < ncell; ++k) g->start[k + 1] += g->start[k];
    uint32_t *fill = (uint32_t *)malloc(sizeof(uint32_t) * (ncell ? ncell : 1));
    if (!fill) return -1;
    memcpy(fill, g->start, sizeof(uint32_t) * ncell);
    for (size_t j = 0; j < nd; ++j)
        if (finite3(dst + 3 * j) && cell_of(g, dst + 3 * j, c)) g->idx[fill[(c[2] * g->n[1] + c[1]) * g->n[0] + c[0]]++] = (uint32_t)j;
    free(fill);
    return 0;
}

static void grid_free(Grid *g) {
    free(g->start);
    free(g->idx);
}

/* nearest target point with d2 < r2; -1 when there is none */
static int64_t nearest(const Grid *g, const double *p, double *d2_out) {
    int64_t c[3], best_j = -1;
    double best = INFINITY;
    if (g->empty || !finite3(p)) return -1;
    /* (a query outside the padded box is farther than h >= radius from every target point) */
    if (!cell_of(g, p, c)) return -1;
    for (int64_t z = c[2] - 1; z <= c[2] + 1; ++z)
        for (int64_t y = c[1] - 1; y <= c[1] + 1; ++y)
            for (int64_t x = c[0] - 1; x <= c[0] + 1; ++x) {
                if (x < 0 || y < 0 || z < 0 || x >= g->n[0] || y >= g->n[1] || z >= g->n[2]) continue;
                const size_t cell = (size_t)((z * g->n[1] + y) * g->n[0] + x);
                for (uint32_t s = g->start[cell]; s < g->start[cell + 1]; ++s) {
                    const int64_t j = g->idx[s];
                    const double dx = p[0] - g->pts[3 * j], dy = p[1] - g->pts[3 * j + 1], dz = p[2] - g->pts[3 * j + 2];
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 < best || (d2 == best && j < best_j)) {
                        best = d2;
                        best_j = j;
                    }
                }
            }
    if (!(best < g->r2)) return -1;
    *d2_out = best;
    return best_j;
}

static void identity4(double *T) {
    for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

static void apply(const double *T, double *p) {
    const double x = p[0], y = p[1], z = p[2];
    p[0] = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    p[1] = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    p[2] = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

static void matmul4(const double *A, const double *B, double *C) {
    double R[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            R[4 * r + c] = ((A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c]) + A[4 * r + 3] * B[12 + c];
    memcpy(C, R, sizeof(R));
}

static void matmul3(const double A[9], const double B[9], double C[9]) {
    double R[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
    memcpy(C, R, sizeof(R));
}

/* rules 2 - 6: the point-to-plane update from the correspondence set */
static void update_plane(const double *mov, size_t ns, const int64_t *corr, const double *dst, const double *nrm, int order,
                         double *U) {
    double A[6][6], b[6];
    size_t count = 0;
    memset(A, 0, sizeof(A));
    memset(b, 0, sizeof(b));
    identity4(U);
    for (size_t t = 0; t < ns; ++t) {
        const size_t i = order >= 0 ? t : ns - 1 - t;
        const int64_t j = corr[i];
        if (j < 0) continue;
        const double *s = mov + 3 * i, *q = dst + 3 * j, *n = nrm + 3 * j;
        const double r = ((s[0] - q[0]) * n[0] + (s[1] - q[1]) * n[1]) + (s[2] - q[2]) * n[2];
        const double J[6] = {s[1] * n[2] - s[2] * n[1], s[2] * n[0] - s[0] * n[2], s[0] * n[1] - s[1] * n[0], n[0], n[1], n[2]};
        for (int a = 0; a < 6; ++a) {
            for (int c = 0; c < 6; ++c) A[a][c] += J[a] * J[c];
            b[a] += J[a] * r;
        }
        ++count;
    }
    if (!count) return;
    /* determinant: elimination with row pivoting */
    double M[6][6], det = 1.0;
    memcpy(M, A, sizeof(M));
    for (int k = 0; k < 6; ++k) {
        int p = k;
        for (int i = k + 1; i < 6; ++i)
            if (fabs(M[i][k]) > fabs(M[p][k])) p = i;
        if (p != k) {
            for (int c = 0; c < 6; ++c) {
                const double t = M[k][c];
                M[k][c] = M[p][c];
                M[p][c] = t;
            }
            det = -det;
        }
        det *= M[k][k];
        if (M[k][k] == 0.0 || M[k][k] != M[k][k]) {
            if (M[k][k] == 0.0) det = det * 0.0;
            break;
        }
        for (int i = k + 1; i < 6; ++i) {
            const double f = M[i][k] / M[k][k];
            for (int c = k; c < 6; ++c) M[i][c] -= f * M[k][c];
        }
    }
    if (!isfinite(det) || fabs(det) < 1e-6) return;
    /* A = L D L^T (A is positive definite here), x = A^-1 (-b) */
    double L[6][6], D[6], x[6];
    memset(L, 0, sizeof(L));
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k] * D[k];
        D[j] = d;
        L[j][j] = 1.0;
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k] * D[k];
            L[i][j] = v / d;
        }
    }
    for (int i = 0; i < 6; ++i) {
        x[i] = -b[i];
        for (int k = 0; k < i; ++k) x[i] -= L[i][k] * x[k];
    }
    for (int i = 0; i < 6; ++i) x[i] /= D[i];
    for (int i = 5; i >= 0; --i)
        for (int k = i + 1; k < 6; ++k) x[i] -= L[k][i] * x[k];
    const double Rx[9] = {1, 0, 0, 0, cos(x[0]), -sin(x[0]), 0, sin(x[0]), cos(x[0])};
    const double Ry[9] = {cos(x[1]), 0, sin(x[1]), 0, 1, 0, -sin(x[1]), 0, cos(x[1])};
    const double Rz[9] = {cos(x[2]), -sin(x[2]), 0, sin(x[2]), cos(x[2]), 0, 0, 0, 1};
    double R[9];
    matmul3(Ry, Rx, R);
    matmul3(Rz, R, R);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) U[4 * r + c] = R[3 * r + c];
        U[4 * r + 3] = x[3 + r];
    }
}

/* the largest eigenvalue's eigenvector of a symmetric 4 x 4 matrix: cyclic Jacobi */
static void max_eigenvector4(double N[4][4], double q[4]) {
    double V[4][4];
    memset(V, 0, sizeof(V));
    for (int k = 0; k < 4; ++k) V[k][k] = 1.0;
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int a = 0; a < 4; ++a)
            for (int c = 0; c < 4; ++c) {
                if (a != c) off += N[a][c] * N[a][c];
                else diag += N[a][c] * N[a][c];
            }
        if (off <= 1e-60 * diag || off == 0.0) break;
        for (int p = 0; p < 3; ++p)
            for (int r = p + 1; r < 4; ++r) {
                if (N[p][r] == 0.0) continue;
                const double theta = (N[r][r] - N[p][p]) / (2.0 * N[p][r]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; ++k) {
                    const double a = N[k][p], b = N[k][r];
                    N[k][p] = c * a - s * b;
                    N[k][r] = s * a + c * b;
                }
                for (int k = 0; k < 4; ++k) {
                    const double a = N[p][k], b = N[r][k];
                    N[p][k] = c * a - s * b;
                    N[r][k] = s * a + c * b;
                }
                for (int k = 0; k < 4; ++k) {
                    const double a = V[k][p], b = V[k][r];
                    V[k][p] = c * a - s * b;
                    V[k][r] = s * a + c * b;
                }
            }
    }
    int m = 0;
    for (int k = 1; k < 4; ++k)
        if (N[k][k] > N[m][m]) m = k;
    for (int k = 0; k < 4; ++k) q[k] = V[k][m];
}

/* TransformationEstimationPointToPoint: the rigid least-squares fit of the correspondence set (Eigen::umeyama, no scale) */
static void update_point(const double *mov, size_t ns, const int64_t *corr, const double *dst, int order, double *U) {
    double ms[3] = {0, 0, 0}, md[3] = {0, 0, 0}, M[3][3];
    size_t count = 0;
    identity4(U);
    for (size_t t = 0; t < ns; ++t) {
        const size_t i = order >= 0 ? t : ns - 1 - t;
        if (corr[i] < 0) continue;
        for (int k = 0; k < 3; ++k) {
            ms[k] += mov[3 * i + k];
            md[k] += dst[3 * corr[i] + k];
        }
        ++count;
    }
    if (!count) return;
    for (int k = 0; k < 3; ++k) {
        ms[k] /= (double)count;
        md[k] /= (double)count;
    }
    memset(M, 0, sizeof(M));
    for (size_t t = 0; t < ns; ++t) {
        const size_t i = order >= 0 ? t : ns - 1 - t;
        if (corr[i] < 0) continue;
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) M[a][c] += (mov[3 * i + a] - ms[a]) * (dst[3 * corr[i] + c] - md[c]);
    }
    double N[4][4] = {{M[0][0] + M[1][1] + M[2][2], M[1][2] - M[2][1], M[2][0] - M[0][2], M[0][1] - M[1][0]},
                      {M[1][2] - M[2][1], M[0][0] - M[1][1] - M[2][2], M[0][1] + M[1][0], M[2][0] + M[0][2]},
                      {M[2][0] - M[0][2], M[0][1] + M[1][0], -M[0][0] + M[1][1] - M[2][2], M[1][2] + M[2][1]},
                      {M[0][1] - M[1][0], M[2][0] + M[0][2], M[1][2] + M[2][1], -M[0][0] - M[1][1] + M[2][2]}};
    double q[4];
    max_eigenvector4(N, q);
    const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] / nq, x = q[1] / nq, y = q[2] / nq, z = q[3] / nq;
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) U[4 * r + c] = R[3 * r + c];
        U[4 * r + 3] = md[r] - ((R[3 * r] * ms[0] + R[3 * r + 1] * ms[1]) + R[3 * r + 2] * ms[2]);
    }
}

/* GetRegistrationResultAndCorrespondences */
static void result(const Grid *g, const double *mov, size_t ns, int order, int64_t *corr, uint64_t *count, double *err2) {
    *count = 0;
    *err2 = 0.0;
    for (size_t i = 0; i < ns; ++i) corr[i] = -1;
    for (size_t t = 0; t < ns; ++t) {
        const size_t i = order >= 0 ? t : ns - 1 - t;
        double d2 = 0.0;
        corr[i] = nearest(g, mov + 3 * i, &d2);
        if (corr[i] >= 0) {
            *err2 += d2;
            ++*count;
        }
    }
}

/* RegistrationICP.  nrm == NULL: point-to-point, else point-to-plane.  T_init: 16 doubles.  Returns 0, -1 out of memory,
 * 1 "Invalid max_correspondence_distance." */
int icp_ref(const double *src, size_t ns, const double *dst, const double *nrm, size_t nd, double max_dist, const double *T_init,
            int max_iteration, double rel_fitness, double rel_rmse, int order, double *T_out, double *fitness, double *rmse,
            uint64_t *count_out, int *iterations, int *converged, int64_t *corr) {
    if (!(max_dist > 0.0)) return 1;
    Grid g;
    if (grid_build(&g, dst, nd, max_dist) != 0) return -1;
    double *mov = (double *)malloc(sizeof(double) * 3 * (ns ? ns : 1));
    if (!mov) return -1;
    double T[16], I4[16];
    identity4(I4);
    memcpy(T, T_init, sizeof(T));
    memcpy(mov, src, sizeof(double) * 3 * ns);
    if (memcmp(T, I4, sizeof(T)) != 0)
        for (size_t i = 0; i < ns; ++i) apply(T, mov + 3 * i);
    uint64_t count;
    double e2;
    result(&g, mov, ns, order, corr, &count, &e2);
    double fit = ns ? (double)count / (double)ns : 0.0, rm = count ? sqrt(e2 / (double)count) : 0.0;
    int it = 0, conv = 0;
    for (; it < max_iteration; ++it) {
        double U[16];
        if (nrm) update_plane(mov, ns, corr, dst, nrm, order, U);
        else update_point(mov, ns, corr, dst, order, U);
        matmul4(U, T, T);
        for (size_t i = 0; i < ns; ++i) apply(U, mov + 3 * i);
        const double fit0 = fit, rm0 = rm;
        result(&g, mov, ns, order, corr, &count, &e2);
        fit = ns ? (double)count / (double)ns : 0.0;
        rm = count ? sqrt(e2 / (double)count) : 0.0;
        if (fabs(fit0 - fit) < rel_fitness && fabs(rm0 - rm) < rel_rmse) {
            ++it;
            conv = 1;
            break;
        }
    }
    memcpy(T_out, T, sizeof(T));
    *fitness = fit;
    *rmse = rm;
    *count_out = count;
    *iterations = it;
    *converged = conv;
    free(mov);
    grid_free(&g);
    return 0;
}

/* the correspondence set of the source under T (GetInformationMatrixFromPointClouds' first step) */
int icp_ref_correspondences(const double *src, size_t ns, const double *dst, size_t nd, double max_dist, const double *T,
                            int64_t *corr) {
    if (!(max_dist > 0.0)) return 1;
    Grid g;
    if (grid_build(&g, dst, nd, max_dist) != 0) return -1;
    for (size_t i = 0; i < ns; ++i) {
        double p[3] = {src[3 * i], src[3 * i + 1], src[3 * i + 2]}, d2;
        apply(T, p);
        corr[i] = nearest(&g, p, &d2);
    }
    grid_free(&g);
    return 0;
}
