/* test_ppf_cluster_fp.c -- a stand-alone run of the PPF pose clustering restatement (ppf_cluster_ref.c) and of the pieces of
 * m3d_ppf_cluster_fp.hpp on small hand cases: meant to be built with -fsanitize=address,undefined (host code only; no GPU, no
 * library).  gcc -O1 -g -ffp-contract=off -fsanitize=address,undefined
 * -static-libasan -static-libubsan test_ppf_cluster_fp.c -lm (the runtimes linked in: the program needs nothing loaded before it).  Prints "ok". */
#include <stdio.h>

#include "ppf_cluster_ref.c"

static int fails = 0;
#define CHECK(c)                                               \
    do {                                                       \
        if (!(c)) {                                            \
            printf("FAILED line %d: %s\n", __LINE__, #c);      \
            ++fails;                                           \
        }                                                      \
    } while (0)

static void pose_at(double *T, double angle_z, double x, double y, double z) {
    const double c = cos(angle_z), s = sin(angle_z);
    const double P[16] = {c, -s, 0, x, s, c, 0, y, 0, 0, 1, z, 0, 0, 0, 1};
    memcpy(T, P, sizeof(P));
}

int main(void) {
    /* K2 */
    CHECK(pcr_threshold(41) == 20 && pcr_threshold(40) == 20 && pcr_threshold(1) == 0 && pcr_threshold(0) == 0);
    CHECK(pc_min_num_pt(0) == 3 && pc_min_num_pt(6) == 3 && pc_min_num_pt(7) == 3 && pc_min_num_pt(8) == 4 && pc_min_num_pt(13) == 6);

    /* MatToQuat / QuatToMat round trip on the four branches */
    {
        const double Rs[4][9] = {{1, 0, 0, 0, 1, 0, 0, 0, 1},
                                 {1 + 2e-16, 0, 0, 0, -1 - 2e-16, 0, 0, 0, -1 - 2e-16},
                                 {-1 - 2e-16, 0, 0, 0, 1 + 2e-16, 0, 0, 0, -1 - 2e-16},
                                 {-1 - 2e-16, 0, 0, 0, -1 - 2e-16, 0, 0, 0, 1 + 2e-16}};
        for (int b = 0; b < 4; ++b) {
            double q[4], R[9];
            pc_mat_to_quat(Rs[b], q);
            pc_quat_to_mat(q, R);
            for (int k = 0; k < 9; ++k) CHECK(fabs(R[k] - Rs[b][k]) < 1e-15);
            CHECK(fabs(q[b]) > 0.99);
        }
    }

    /* Jacobi: a matrix with known eigenvalues 1, 2, 3, 4 in a rotated basis, and a diagonal one */
    {
        double A[16] = {4, 0, 0, 0, 0, 1, 0, 0, 0, 0, 3, 0, 0, 0, 0, 2}, w[4], V[16];
        pc_jacobi4(A, w, V);
        CHECK(w[0] == 4 && w[1] == 1 && w[2] == 3 && w[3] == 2 && V[0] == 1 && V[5] == 1);
        double B[16] = {2.5, 0.5, 0, 0, 0.5, 2.5, 0, 0, 0, 0, 1, 0, 0, 0, 0, 4};   /* eigenvalues 3, 2, 1, 4 */
        pc_jacobi4(B, w, V);
        double sum = 0, prod = 1;
        for (int i = 0; i < 4; ++i) {
            sum += w[i];
            prod *= w[i];
        }
        CHECK(fabs(sum - 10) < 1e-14 && fabs(prod - 24) < 1e-13);
    }

    /* K1 - K6: five poses on a line 0.6 r apart and two stragglers; two of the votes below the cut */
    {
        enum { P = 9 };
        double poses[16 * P], avg[16 * P];
        const uint32_t votes[P] = {50, 49, 48, 47, 46, 45, 44, 10, 9};
        const double r = 0.05;
        for (int k = 0; k < 5; ++k) pose_at(poses + 16 * k, 0.3, 0.6 * r * k, 0, 0);
        pose_at(poses + 16 * 5, 0.3, 1.0, 0, 0);
        pose_at(poses + 16 * 6, 2.0, 0.6 * r, 0, 0);   /* in the cluster by translation, 97 degrees off by rotation */
        pose_at(poses + 16 * 7, 0.3, 0, 0, 0);         /* cut by K2 */
        pose_at(poses + 16 * 8, 0.3, 0, 0, 0);
        uint32_t order[P], count_t[P], count_r[P], avg_cluster[P];
        int32_t label_t[P], label_r[P], min_t, min_r[P];
        uint64_t cvotes[P], avotes[P], counts[2];
        const size_t n = pcr_cluster(poses, votes, P, r, 12.0 / 180.0 * M_PI, order, count_t, label_t, count_r, label_r, &min_t, min_r,
                                     cvotes, avg, avotes, avg_cluster, counts);
        CHECK(n == 7 && counts[0] == 1 && counts[1] == 1 && min_t == 3 && min_r[0] == 3);
        const uint32_t want_t[7] = {3, 4, 4, 3, 2, 1, 4};
        const int32_t want_lt[7] = {0, 0, 0, 0, 0, -1, 0}, want_lr[7] = {0, 0, 0, 0, 0, -1, -1};
        for (int i = 0; i < 7; ++i) CHECK(order[i] == (uint32_t)i && count_t[i] == want_t[i] && label_t[i] == want_lt[i] && label_r[i] == want_lr[i]);
        CHECK(cvotes[0] == 50 + 49 + 48 + 47 + 46 + 44 && avotes[0] == 240 && avg_cluster[0] == 0);
        CHECK(fabs(avg[3] - 1.2 * r) < 1e-15 && fabs(avg[0] - cos(0.3)) < 1e-14 && fabs(avg[4] - sin(0.3)) < 1e-14);
        /* nothing at all, and a single pose */
        CHECK(pcr_cluster(poses, votes, 0, r, 0.2, order, count_t, label_t, count_r, label_r, &min_t, min_r, cvotes, avg, avotes, avg_cluster, counts) == 0);
        CHECK(pcr_cluster(poses, votes, 1, r, 0.2, order, count_t, label_t, count_r, label_r, &min_t, min_r, cvotes, avg, avotes, avg_cluster, counts) == 1 &&
              counts[0] == 0 && label_t[0] == -1);
    }

    /* K8 */
    {
        double T[48], q[12], t[9], s[3];
        uint64_t v[3] = {12, 30, 6};
        const double c[3] = {0.5, 0.25, 0.125};
        pose_at(T, 0, 1, 2, 3);
        pose_at(T + 16, 0, 4, 5, 6);
        pose_at(T + 32, 0, 7, 8, 9);
        CHECK(pcr_finish(T, v, 3, c, 0.6, 10, 0.6, 10, q, t, s) == 2);
        CHECK(v[0] == 30 && v[1] == 12 && s[0] == 1.0 && s[1] == 12 / 15.0 && t[0] == 3.5 && t[3] == 0.5 && q[0] == 1.0);
        CHECK(pcr_finish(T, v, 0, c, 0.6, 10, 0.6, 10, q, t, s) == 0);
    }
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
