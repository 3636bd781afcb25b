// m3d_ppf_cluster_fp.hpp -- the arithmetic of the PPF pose clustering (include/misc3d_amd.h, "PPF pose clustering"): the ONE
// place the pair distance, the rotation trace, the two match predicates, MatToQuat / QuatToMat, the 4 x 4 Jacobi solver, the
// centre shift and the score exist.  Written in the common subset of C and C++ and with no HIP in it: the kernels
// (m3d_ppf_cluster.hip), the host driver (m3d_ppf_cluster.cpp) and the serial restatement (tests/cpp/ppf_cluster_ref.c, a C
// file) compile this one text.  Build with -ffp-contract=off; every sum is written out with its association, and divisions and
// square roots are the correctly rounded fp64 ones.  A pose is 16 doubles, row-major 4 x 4.
#ifndef M3D_PPF_CLUSTER_FP_HPP
#define M3D_PPF_CLUSTER_FP_HPP
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define M3D_PC_HD static __host__ __device__ __forceinline__
#else
#define M3D_PC_HD static inline
#endif

/* K3: d2 = (dx dx + dy dy) + dz dz */
M3D_PC_HD double pc_d2(double dx, double dy, double dz) { return (dx * dx + dy * dy) + dz * dz; }

/* K5: the serial sum of the nine products src(r, c) dst(r, c), row-major (a, b: the nine rotation entries) */
M3D_PC_HD double pc_trace(const double *a, const double *b) {
    double trace = 0;
    for (int k = 0; k < 9; ++k) trace += a[k] * b[k];
    return trace;
}
M3D_PC_HD double pc_ca(double trace) { return (trace - 1) / 2; }

/* the two match relations: K3 (translation) and K5 (translation and rotation); r2 = r * r and cos_edge = cos(angle_threshold)
 * are computed once on the host.  acos(ca) < thr is ca > cos(thr); the reference's clamps at |ca| > 1 fall out of the compare. */
M3D_PC_HD int pc_match_t(double d2, double r2) { return d2 < r2; }
M3D_PC_HD int pc_match_tr(double d2, double r2, double ca, double cos_edge) { return d2 < r2 && ca > cos_edge; }

/* K4: int(max(6, the largest neighbour count) / 2.0) */
M3D_PC_HD uint32_t pc_min_num_pt(uint32_t max_count) { return (max_count > 6u ? max_count : 6u) / 2u; }

/* MatToQuat (data_structure.h:58-87); R: the nine rotation entries row-major; q = (w, x, y, z) */
M3D_PC_HD void pc_mat_to_quat(const double *R, double *q) {
    const double tr = (R[0] + R[4]) + R[8];
    double s;
    if (tr > -1) {
        s = sqrt(tr + 1) * 2;
        q[0] = 0.25 * s;
        q[1] = (R[7] - R[5]) / s;
        q[2] = (R[2] - R[6]) / s;
        q[3] = (R[3] - R[1]) / s;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        s = sqrt(((1 + R[0]) - R[4]) - R[8]) * 2;
        q[0] = (R[7] - R[5]) / s;
        q[1] = 0.25 * s;
        q[2] = (R[1] + R[3]) / s;
        q[3] = (R[2] + R[6]) / s;
    } else if (R[4] > R[8]) {
        s = sqrt(((1 + R[4]) - R[0]) - R[8]) * 2;
        q[0] = (R[2] - R[6]) / s;
        q[1] = (R[1] + R[3]) / s;
        q[2] = 0.25 * s;
        q[3] = (R[5] + R[7]) / s;
    } else {
        s = sqrt(((1 + R[8]) - R[0]) - R[4]) * 2;
        q[0] = (R[3] - R[1]) / s;
        q[1] = (R[2] + R[6]) / s;
        q[2] = (R[5] + R[7]) / s;
        q[3] = 0.25 * s;
    }
}

/* QuatToMat (data_structure.h:40-50) */
M3D_PC_HD void pc_quat_to_mat(const double *q, double *R) {
    R[0] = 1 - 2 * (q[2] * q[2] + q[3] * q[3]);
    R[1] = 2 * (q[1] * q[2] - q[0] * q[3]);
    R[2] = 2 * (q[0] * q[2] + q[1] * q[3]);
    R[3] = 2 * (q[1] * q[2] + q[0] * q[3]);
    R[4] = 1 - 2 * (q[1] * q[1] + q[3] * q[3]);
    R[5] = 2 * (q[2] * q[3] - q[0] * q[1]);
    R[6] = 2 * (q[1] * q[3] - q[0] * q[2]);
    R[7] = 2 * (q[0] * q[1] + q[2] * q[3]);
    R[8] = 1 - 2 * (q[1] * q[1] + q[2] * q[2]);
}

M3D_PC_HD void pc_pose_rotation(const double *pose, double *R) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = pose[4 * r + c];
}

/* K6: the running sums of one sub-cluster: the 10 distinct entries of sum q q^T (row-major upper triangle), sum t, the count */
typedef struct pc_avg_sums {
    double qq[10];
    double t[3];
    uint64_t votes;
    uint64_t count;
} pc_avg_sums;

M3D_PC_HD void pc_avg_clear(pc_avg_sums *S) {
    for (int k = 0; k < 10; ++k) S->qq[k] = 0.0;
    S->t[0] = S->t[1] = S->t[2] = 0.0;
    S->votes = 0;
    S->count = 0;
}
M3D_PC_HD void pc_avg_add(pc_avg_sums *S, const double *pose, uint32_t votes) {
    double R[9], q[4];
    int k = 0;
    pc_pose_rotation(pose, R);
    pc_mat_to_quat(R, q);
    for (int a = 0; a < 4; ++a)
        for (int b = a; b < 4; ++b) S->qq[k++] += q[a] * q[b];
    for (int a = 0; a < 3; ++a) S->t[a] += pose[4 * a + 3];
    S->votes += votes;
    S->count += 1;
}

/* Cyclic Jacobi for a symmetric 4 x 4 (A row-major, destroyed): eigenvalues in w, eigenvectors in the COLUMNS of V.  Sweeps
 * over (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) until every off-diagonal entry is exactly zero, at most 64 sweeps. */
M3D_PC_HD void pc_jacobi4(double *A, double *w, double *V) {
    for (int i = 0; i < 16; ++i) V[i] = 0.0;
    for (int i = 0; i < 4; ++i) V[5 * i] = 1.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) off += fabs(A[4 * p + q]);
        if (off == 0.0) break;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[4 * p + q];
                if (apq == 0.0) continue;
                const double app = A[5 * p], aqq = A[5 * q];
                /* an entry that no longer changes either diagonal neighbour is set to zero (Rutishauser) */
                if (fabs(app) + fabs(apq) * 100.0 == fabs(app) && fabs(aqq) + fabs(apq) * 100.0 == fabs(aqq) && sweep > 3) {
                    A[4 * p + q] = A[4 * q + p] = 0.0;
                    continue;
                }
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                A[5 * p] = app - t * apq;
                A[5 * q] = aqq + t * apq;
                A[4 * p + q] = A[4 * q + p] = 0.0;
                for (int k = 0; k < 4; ++k) {
                    if (k != p && k != q) {
                        const double akp = A[4 * k + p], akq = A[4 * k + q];
                        A[4 * k + p] = A[4 * p + k] = c * akp - s * akq;
                        A[4 * k + q] = A[4 * q + k] = s * akp + c * akq;
                    }
                    const double vkp = V[4 * k + p], vkq = V[4 * k + q];
                    V[4 * k + p] = c * vkp - s * vkq;
                    V[4 * k + q] = s * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < 4; ++i) w[i] = A[5 * i];
}

/* K6: the averaged pose of a sub-cluster from its sums: the eigenvector of the largest eigenvalue (the first on ties), signed so
 * that its component of largest magnitude (lowest index on ties) is positive; t_avg = sum * (1.0 / count) */
M3D_PC_HD void pc_avg_pose(const pc_avg_sums *S, double *pose, double *q_out) {
    double A[16], w[4], V[16], q[4];
    int k = 0, best = 0, big = 0;
    for (int a = 0; a < 4; ++a)
        for (int b = a; b < 4; ++b) {
            A[4 * a + b] = S->qq[k];
            A[4 * b + a] = S->qq[k];
            ++k;
        }
    pc_jacobi4(A, w, V);
    for (int i = 1; i < 4; ++i)
        if (w[i] > w[best]) best = i;
    for (int i = 0; i < 4; ++i) q[i] = V[4 * i + best];
    for (int i = 1; i < 4; ++i)
        if (fabs(q[i]) > fabs(q[big])) big = i;
    if (q[big] < 0.0)
        for (int i = 0; i < 4; ++i) q[i] = -q[i];
    double R[9];
    pc_quat_to_mat(q, R);
    const double inv = 1.0 / (double)S->count;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) pose[4 * r + c] = R[3 * r + c];
        pose[4 * r + 3] = S->t[r] * inv;
    }
    pose[12] = pose[13] = pose[14] = 0.0;
    pose[15] = 1.0;
    if (q_out)
        for (int i = 0; i < 4; ++i) q_out[i] = q[i];
}

/* K8: the centre shift T(i, 3) -= (c0 T(i, 0) + c1 T(i, 1)) + c2 T(i, 2) */
M3D_PC_HD void pc_centre_shift(double *pose, const double *c) {
    for (int i = 0; i < 3; ++i) pose[4 * i + 3] -= (c[0] * pose[4 * i] + c[1] * pose[4 * i + 1]) + c[2] * pose[4 * i + 2];
}

/* K8: expected = ((ratio n) n) 0.25, score = min(1.0, votes / expected) */
M3D_PC_HD double pc_expected_votes(double ratio, uint64_t n) { return ((ratio * (double)n) * (double)n) * 0.25; }
/* EdgePoints mode (rule E9): reference_num_ refered_num_ are both the sample's size, and no reduction factor */
M3D_PC_HD double pc_expected_votes_edges(double ratio, uint64_t n) { return (ratio * (double)n) * (double)n; }
M3D_PC_HD double pc_score(uint64_t votes, double expected) {
    const double s = (double)votes / expected;
    return s < 1.0 ? s : 1.0;
}

#endif /* M3D_PPF_CLUSTER_FP_HPP */
