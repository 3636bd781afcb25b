/* colored_icp_ref.c -- a plain-C, one-thread restatement of the coloured ICP contract of include/misc3d_amd.h
 * (m3d_color_gradient, m3d_registration_icp_colored): Open3D 0.15.1 RegistrationColoredICP, restated from the numbered rules
 * G1 - G7 and C1 - C6 there.  The checker of the GPU tests; built by tests/colored_icp_ref_util.py with gcc -O2
 * -ffp-contract=off.  The correspondence search, the pose update of a cloud and the outer loop's helpers are icp_ref.c's (its
 * text is included below: one restatement of GetRegistrationResultAndCorrespondences for all three estimators).  Its own:
 *   - the Hybrid neighbour lists: brute force over all target points, insertion by (d2, index);
 *   - the gradient's rows and serial sums, and a 3 x 3 LDL^T with Eigen's diagonal pivoting written for this size;
 *   - the two rows per correspondence, serial sums over the source index (ascending: order >= 0, descending: order < 0), its
 *     own 6 x 6 elimination for the determinant, an unpivoted LDL^T for the solve, the rotation as three matrices.
 */
#include "icp_ref.c"

#define CG_MAXNN 128

static double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

static double intensity(const double *c) { return ((c[0] + c[1]) + c[2]) / 3.0; }

/* G1: up to max_nn nearest by (d2, index) among the finite target points, d2 < r2; returns nn */
static int hybrid_list(const double *xyz, size_t n, size_t k, double r2, int max_nn, int64_t *idx, double *dd) {
    int m = 0;
    const double *q = xyz + 3 * k;
    if (!finite3(q)) return 0;
    for (size_t j = 0; j < n; ++j) {
        const double *p = xyz + 3 * j;
        if (!finite3(p)) continue;
        const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (!isfinite(d2) || !(d2 < r2)) continue;
        if (m == max_nn && !(d2 < dd[m - 1])) continue; /* j ascends: an equal d2 with a larger index loses */
        int t = m < max_nn ? m++ : max_nn - 1;
        while (t > 0 && d2 < dd[t - 1]) {
            dd[t] = dd[t - 1];
            idx[t] = idx[t - 1];
            --t;
        }
        dd[t] = d2;
        idx[t] = (int64_t)j;
    }
    return m;
}

/* G7: x = LDLT(A).solve(b), A symmetric 3 x 3: the largest remaining |diagonal| is the pivot of every step (the first on
 * ties), a zero pivot's component is 0 */
static void ldlt3(const double A[3][3], const double b[3], double x[3]) {
    double M[3][3], D[3], y[3];
    int perm[3] = {0, 1, 2};
    memcpy(M, A, sizeof(M));
    for (int k = 0; k < 3; ++k) {
        int p = k;
        for (int i = k + 1; i < 3; ++i)
            if (fabs(M[i][i]) > fabs(M[p][p])) p = i;
        if (p != k) {
            for (int j = 0; j < 3; ++j) {
                const double t = M[k][j];
                M[k][j] = M[p][j];
                M[p][j] = t;
            }
            for (int i = 0; i < 3; ++i) {
                const double t = M[i][k];
                M[i][k] = M[i][p];
                M[i][p] = t;
            }
            const int t = perm[k];
            perm[k] = perm[p];
            perm[p] = t;
        }
        D[k] = M[k][k];
        for (int i = k + 1; i < 3; ++i) {
            const double l = D[k] != 0.0 ? M[i][k] / D[k] : 0.0;
            for (int j = k + 1; j < 3; ++j) M[i][j] -= l * M[k][j];
            M[i][k] = l;
        }
    }
    for (int i = 0; i < 3; ++i) y[i] = b[perm[i]];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < i; ++j) y[i] -= M[i][j] * y[j];
    for (int i = 0; i < 3; ++i) y[i] = D[i] != 0.0 ? y[i] / D[i] : 0.0;
    for (int i = 2; i >= 0; --i)
        for (int j = i + 1; j < 3; ++j) y[i] -= M[j][i] * y[j];
    for (int i = 0; i < 3; ++i) x[perm[i]] = y[i];
}

/* G1 - G7.  grad: n x 3; nn_out (may be NULL): the list lengths; ata_out (n x 9, may be NULL): AtA of every point, zeros
 * where nn < 4.  Returns 0, 1 max_nn out of range, -1 out of memory */
int colored_ref_gradient(const double *xyz, const double *nrm, const double *col, size_t n, double radius, int max_nn, double *grad,
                         int32_t *nn_out, double *ata_out) {
    if (max_nn < 1 || max_nn > CG_MAXNN) return 1;
    const double r2 = radius * radius;
    double *I = (double *)malloc(sizeof(double) * (n ? n : 1));
    if (!I) return -1;
    for (size_t k = 0; k < n; ++k) I[k] = intensity(col + 3 * k);
    for (size_t k = 0; k < n; ++k) {
        int64_t L[CG_MAXNN];
        double dd[CG_MAXNN];
        const int nn = hybrid_list(xyz, n, k, r2, max_nn, L, dd);
        double g[3] = {0.0, 0.0, 0.0};
        double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, b[3] = {0, 0, 0};
        if (nn_out) nn_out[k] = nn;
        if (nn >= 4) {
            const double *v = xyz + 3 * k, *nk = nrm + 3 * k;
            for (int i = 1; i <= nn; ++i) {
                double a[3], bi;
                if (i < nn) {
                    const double *p = xyz + 3 * L[i];
                    const double d[3] = {p[0] - v[0], p[1] - v[1], p[2] - v[2]};
                    const double s = dot3(d, nk);
                    for (int c = 0; c < 3; ++c) a[c] = (p[c] - s * nk[c]) - v[c];
                    bi = I[L[i]] - I[k];
                } else { /* G5 */
                    for (int c = 0; c < 3; ++c) a[c] = (double)(nn - 1) * nk[c];
                    bi = 0.0;
                }
                for (int r = 0; r < 3; ++r) {
                    for (int c = r; c < 3; ++c) A[r][c] += a[r] * a[c];
                    b[r] += a[r] * bi;
                }
            }
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < r; ++c) A[r][c] = A[c][r];
            ldlt3(A, b, g);
        }
        if (ata_out) memcpy(ata_out + 9 * k, A, sizeof(A));
        memcpy(grad + 3 * k, g, sizeof(g));
    }
    free(I);
    return 0;
}

/* C1 - C6: the update from the correspondence set */
static void update_colored(const double *mov, size_t ns, const int64_t *corr, const double *Is, const double *dst, const double *nrm,
                           const double *grad, const double *It, double sg, double sp, int order, double *U) {
    double A[6][6], b[6];
    size_t count = 0;
    memset(A, 0, sizeof(A));
    memset(b, 0, sizeof(b));
    identity4(U);
    for (size_t t = 0; t < ns; ++t) {
        const size_t i = order >= 0 ? t : ns - 1 - t;
        const int64_t j = corr[i];
        if (j < 0) continue;
        const double *s = mov + 3 * i, *q = dst + 3 * j, *n = nrm + 3 * j, *g = grad + 3 * j;
        const double d[3] = {s[0] - q[0], s[1] - q[1], s[2] - q[2]};
        const double e = dot3(d, n);
        const double r0 = sg * e;
        const double J0[6] = {sg * (s[1] * n[2] - s[2] * n[1]), sg * (s[2] * n[0] - s[0] * n[2]), sg * (s[0] * n[1] - s[1] * n[0]),
                              sg * n[0], sg * n[1], sg * n[2]};
        double qq[3], M[3][3], m[3];
        for (int c = 0; c < 3; ++c) qq[c] = (s[c] - e * n[c]) - q[c];
        const double I0 = dot3(g, qq) + It[j];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) M[r][c] = r == c ? 1.0 - n[r] * n[c] : -(n[r] * n[c]);
        for (int c = 0; c < 3; ++c) m[c] = -((g[0] * M[0][c] + g[1] * M[1][c]) + g[2] * M[2][c]);
        const double J1[6] = {sp * (s[1] * m[2] - s[2] * m[1]), sp * (s[2] * m[0] - s[0] * m[2]), sp * (s[0] * m[1] - s[1] * m[0]),
                              sp * m[0], sp * m[1], sp * m[2]};
        const double r1 = sp * (Is[i] - I0);
        for (int a = 0; a < 6; ++a) {
            for (int c = 0; c < 6; ++c) A[a][c] += J0[a] * J0[c] + J1[a] * J1[c];
            b[a] += J0[a] * r0 + J1[a] * r1;
        }
        ++count;
    }
    if (!count) return;
    /* determinant: elimination with row pivoting */
    double E[6][6], det = 1.0;
    memcpy(E, A, sizeof(E));
    for (int k = 0; k < 6; ++k) {
        int p = k;
        for (int i = k + 1; i < 6; ++i)
            if (fabs(E[i][k]) > fabs(E[p][k])) p = i;
        if (p != k) {
            for (int c = 0; c < 6; ++c) {
                const double t = E[k][c];
                E[k][c] = E[p][c];
                E[p][c] = t;
            }
            det = -det;
        }
        det *= E[k][k];
        if (E[k][k] == 0.0 || E[k][k] != E[k][k]) {
            if (E[k][k] == 0.0) det = det * 0.0;
            break;
        }
        for (int i = k + 1; i < 6; ++i) {
            const double f = E[i][k] / E[k][k];
            for (int c = k; c < 6; ++c) E[i][c] -= f * E[k][c];
        }
    }
    if (!isfinite(det) || fabs(det) < 1e-6) return;
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

/* RegistrationColoredICP.  Returns 0, -1 out of memory, 1 "Invalid max_correspondence_distance.", 2 lambda outside [0, 1] */
int colored_ref_icp(const double *src, const double *src_col, size_t ns, const double *dst, const double *nrm, const double *dst_col,
                    size_t nd, double max_dist, double lambda, const double *T_init, int max_iteration, double rel_fitness,
                    double rel_rmse, int order, double *T_out, double *fitness, double *rmse, uint64_t *count_out, int *iterations,
                    int *converged, int64_t *corr) {
    if (!(max_dist > 0.0)) return 1;
    if (!(lambda >= 0.0 && lambda <= 1.0)) return 2;
    const double sg = sqrt(lambda), sp = sqrt(1.0 - lambda);
    Grid g;
    if (grid_build(&g, dst, nd, max_dist) != 0) return -1;
    double *mov = (double *)malloc(sizeof(double) * 3 * (ns ? ns : 1));
    double *grad = (double *)malloc(sizeof(double) * 3 * (nd ? nd : 1));
    double *It = (double *)malloc(sizeof(double) * (nd ? nd : 1));
    double *Is = (double *)malloc(sizeof(double) * (ns ? ns : 1));
    if (!mov || !grad || !It || !Is) return -1;
    if (colored_ref_gradient(dst, nrm, dst_col, nd, 2.0 * max_dist, 30, grad, NULL, NULL) != 0) return -1;
    for (size_t j = 0; j < nd; ++j) It[j] = intensity(dst_col + 3 * j);
    for (size_t i = 0; i < ns; ++i) Is[i] = intensity(src_col + 3 * i);
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
        update_colored(mov, ns, corr, Is, dst, nrm, grad, It, sg, sp, order, U);
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
    free(grad);
    free(It);
    free(Is);
    grid_free(&g);
    return 0;
}
