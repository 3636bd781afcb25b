/* ppf_cluster_ref.c -- the contract "PPF pose clustering" of include/misc3d_amd.h restated in serial C: K1 - K6 (pcr_cluster) and
 * K8 (pcr_finish).  K7 is the ICP restatements' (tests/cpp/icp_ref.c, tests/icp_l1_ref_util.py; tests/ppf_cluster_ref_util.py
 * puts the three together).  It shares with the library only the arithmetic both must share, m3d_ppf_cluster_fp.hpp: the
 * clusters are found by a plain breadth-first walk over the cores in ascending order, not by a union-find.
 * gcc -O2 -ffp-contract=off [-fopenmp: the two counting loops]. */
#include <stdlib.h>
#include <string.h>

#include "../../misc3d_amd/csrc/m3d_ppf_cluster_fp.hpp"

typedef struct {
    const double *poses;    /* the caller's, 16 each */
    const uint32_t *order;  /* sorted position -> input index */
    const uint32_t *votes;  /* by sorted position */
    double r2, cos_edge;
} Ctx;

static const double *pose_of(const Ctx *c, uint32_t i) { return c->poses + 16 * (size_t)c->order[i]; }

static int match(const Ctx *c, uint32_t i, uint32_t j, int level) {
    const double *a = pose_of(c, i), *b = pose_of(c, j);
    const double d2 = pc_d2(b[3] - a[3], b[7] - a[7], b[11] - a[11]);
    if (level == 1) return pc_match_t(d2, c->r2);
    double Ra[9], Rb[9];
    pc_pose_rotation(a, Ra);
    pc_pose_rotation(b, Rb);
    return pc_match_tr(d2, c->r2, pc_ca(pc_trace(Ra, Rb)), c->cos_edge);
}

typedef struct {
    uint64_t votes;
    uint32_t lowest, id;
} Cluster;

static int by_votes(const void *x, const void *y) {
    const Cluster *a = (const Cluster *)x, *b = (const Cluster *)y;
    if (a->votes != b->votes) return a->votes > b->votes ? -1 : 1;
    return a->lowest < b->lowest ? -1 : (a->lowest > b->lowest ? 1 : 0);
}

/* K4 over the members idx[0 .. k) (ascending sorted positions) under the level's relation.  count[m], rank[m] (the rank of
 * member m's cluster, -1 = dropped) per member; -> the number of clusters, their votes in rank order in cl_votes (k entries). */
static size_t gather(const Ctx *c, const uint32_t *idx, size_t k, int level, uint32_t *count, int32_t *rank, int32_t *min_num_pt,
                     uint64_t *cl_votes) {
    uint32_t max_count = 0;
    long m;
#pragma omp parallel for schedule(dynamic, 16)
    for (m = 0; m < (long)k; ++m) {
        uint32_t n = 0;
        for (size_t o = 0; o < k; ++o) n += match(c, idx[m], idx[o], level) ? 1u : 0u;
        count[m] = n;
    }
    for (size_t a = 0; a < k; ++a)
        if (count[a] > max_count) max_count = count[a];
    const uint32_t min_pt = pc_min_num_pt(max_count);
    *min_num_pt = (int32_t)min_pt;
    int32_t *comp = (int32_t *)malloc(sizeof(int32_t) * (k ? k : 1));
    uint32_t *queue = (uint32_t *)malloc(sizeof(uint32_t) * (k ? k : 1));
    for (size_t a = 0; a < k; ++a) comp[a] = -1;
    size_t n_comp = 0;
    for (size_t s = 0; s < k; ++s) {   /* a cluster starts at its lowest core */
        if (comp[s] >= 0 || count[s] < min_pt) continue;
        size_t head = 0, tail = 0;
        queue[tail++] = (uint32_t)s;
        comp[s] = (int32_t)n_comp;
        while (head < tail) {
            const uint32_t a = queue[head++];
            for (size_t b = 0; b < k; ++b)
                if (comp[b] < 0 && count[b] >= min_pt && match(c, idx[a], idx[b], level)) {
                    comp[b] = (int32_t)n_comp;
                    queue[tail++] = (uint32_t)b;
                }
        }
        ++n_comp;
    }
    /* a non-core pose joins the cluster that starts first among those of its core neighbours */
    int32_t *joined = (int32_t *)malloc(sizeof(int32_t) * (k ? k : 1));
#pragma omp parallel for schedule(dynamic, 16)
    for (m = 0; m < (long)k; ++m) {
        int32_t best = comp[m];
        if (count[m] < min_pt) {
            best = -1;
            for (size_t b = 0; b < k; ++b)
                if (count[b] >= min_pt && (best < 0 || comp[b] < best) && match(c, idx[m], idx[b], level)) best = comp[b];
        }
        joined[m] = best;
    }
    Cluster *cl = (Cluster *)calloc(n_comp ? n_comp : 1, sizeof(Cluster));
    for (size_t a = 0; a < n_comp; ++a) {
        cl[a].id = (uint32_t)a;
        cl[a].lowest = 0xFFFFFFFFu;
    }
    for (size_t a = 0; a < k; ++a)
        if (joined[a] >= 0) {
            Cluster *x = &cl[joined[a]];
            x->votes += c->votes[idx[a]];
            if (x->lowest == 0xFFFFFFFFu) x->lowest = idx[a];
        }
    qsort(cl, n_comp, sizeof(Cluster), by_votes);
    int32_t *rank_of = (int32_t *)malloc(sizeof(int32_t) * (n_comp ? n_comp : 1));
    for (size_t a = 0; a < n_comp; ++a) {
        rank_of[cl[a].id] = (int32_t)a;
        cl_votes[a] = cl[a].votes;
    }
    for (size_t a = 0; a < k; ++a) rank[a] = joined[a] >= 0 ? rank_of[joined[a]] : -1;
    free(rank_of);
    free(cl);
    free(joined);
    free(queue);
    free(comp);
    return n_comp;
}

static const uint32_t *g_votes;
static int by_pose_votes(const void *x, const void *y) {
    const uint32_t a = *(const uint32_t *)x, b = *(const uint32_t *)y;
    if (g_votes[a] != g_votes[b]) return g_votes[a] > g_votes[b] ? -1 : 1;
    return a < b ? -1 : (a > b ? 1 : 0);
}

/* K2 alone */
size_t pcr_threshold(uint32_t max_votes) { return (size_t)((double)max_votes * 0.5); }

/* K1 - K6.  Every per-pose and per-cluster array holds P entries (avg_poses 16 P).  counts[0] = translation clusters,
 * counts[1] = sub-clusters.  -> the number of valid poses. */
size_t pcr_cluster(const double *poses, const uint32_t *votes, size_t P, double dist_threshold, double angle_threshold, uint32_t *order,
                   uint32_t *count_t, int32_t *label_t, uint32_t *count_r, int32_t *label_r, int32_t *min_num_pt_t,
                   int32_t *min_num_pt_r, uint64_t *cluster_votes, double *avg_poses, uint64_t *avg_votes, uint32_t *avg_cluster,
                   uint64_t *counts) {
    counts[0] = counts[1] = 0;
    *min_num_pt_t = 0;
    if (P == 0) return 0;
    uint32_t *all = (uint32_t *)malloc(sizeof(uint32_t) * P);
    for (size_t i = 0; i < P; ++i) all[i] = (uint32_t)i;
    g_votes = votes;
    qsort(all, P, sizeof(uint32_t), by_pose_votes);
    const size_t threshold = pcr_threshold(votes[all[0]]);
    size_t V = 0;
    while (V < P && votes[all[V]] >= threshold) ++V;
    memcpy(order, all, sizeof(uint32_t) * V);
    uint32_t *sv = (uint32_t *)malloc(sizeof(uint32_t) * V), *idx = (uint32_t *)malloc(sizeof(uint32_t) * V);
    for (size_t i = 0; i < V; ++i) {
        sv[i] = votes[order[i]];
        idx[i] = (uint32_t)i;
        count_r[i] = 0;
        label_r[i] = -1;
    }
    Ctx c = {poses, order, sv, dist_threshold * dist_threshold, cos(angle_threshold)};
    const size_t n_t = gather(&c, idx, V, 1, count_t, label_t, min_num_pt_t, cluster_votes);
    counts[0] = n_t;
    uint32_t *cnt = (uint32_t *)malloc(sizeof(uint32_t) * (V ? V : 1));
    int32_t *rk = (int32_t *)malloc(sizeof(int32_t) * (V ? V : 1));
    uint64_t *cv = (uint64_t *)malloc(sizeof(uint64_t) * (V ? V : 1));
    size_t n_avg = 0;
    for (size_t t = 0; t < n_t; ++t) {
        size_t k = 0;
        for (size_t i = 0; i < V; ++i)
            if (label_t[i] == (int32_t)t) idx[k++] = (uint32_t)i;
        const size_t n_r = gather(&c, idx, k, 2, cnt, rk, &min_num_pt_r[t], cv);
        for (size_t a = 0; a < k; ++a) {
            count_r[idx[a]] = cnt[a];
            label_r[idx[a]] = rk[a];
        }
        for (size_t s = 0; s < n_r; ++s) {   /* K6, members ascending */
            pc_avg_sums S;
            pc_avg_clear(&S);
            for (size_t a = 0; a < k; ++a)
                if (rk[a] == (int32_t)s) pc_avg_add(&S, pose_of(&c, idx[a]), sv[idx[a]]);
            pc_avg_pose(&S, avg_poses + 16 * n_avg, 0);
            avg_votes[n_avg] = S.votes;
            avg_cluster[n_avg] = (uint32_t)t;
            ++n_avg;
        }
    }
    counts[1] = n_avg;
    free(cv);
    free(rk);
    free(cnt);
    free(idx);
    free(sv);
    free(all);
    return V;
}

/* K8 on k refined poses (16 doubles each) with their votes, in translation-cluster order: the centre shift, the stable sort, the
 * score, the two cuts.  poses and votes are reordered in place; q (4 k), t (3 k), scores (k) are filled for the kept ones.
 * -> the number of results kept. */
size_t pcr_finish(double *poses, uint64_t *votes, size_t k, const double *centroid, double ratio, uint64_t n_model, double score_thresh,
                  int num_result, double *q, double *t, double *scores) {
    for (size_t i = 0; i < k; ++i) pc_centre_shift(poses + 16 * i, centroid);
    for (size_t i = 1; i < k; ++i) {   /* insertion sort: stable */
        double T[16];
        const uint64_t v = votes[i];
        memcpy(T, poses + 16 * i, sizeof(T));
        size_t j = i;
        while (j > 0 && votes[j - 1] < v) {
            votes[j] = votes[j - 1];
            memcpy(poses + 16 * j, poses + 16 * (j - 1), sizeof(T));
            --j;
        }
        votes[j] = v;
        memcpy(poses + 16 * j, T, sizeof(T));
    }
    const double expected = pc_expected_votes(ratio, n_model);
    size_t keep = 0;
    while (keep < k && !(pc_score(votes[keep], expected) < score_thresh)) ++keep;
    if (num_result >= 0 && keep > (size_t)num_result) keep = (size_t)num_result;
    for (size_t i = 0; i < keep; ++i) {
        double R[9];
        pc_pose_rotation(poses + 16 * i, R);
        pc_mat_to_quat(R, q + 4 * i);
        for (int a = 0; a < 3; ++a) t[3 * i + a] = poses[16 * i + 4 * a + 3];
        scores[i] = pc_score(votes[i], expected);
    }
    return keep;
}

/* the header's pieces, for the tests */
void pcr_mat_to_quat(const double *R, double *q) { pc_mat_to_quat(R, q); }
void pcr_quat_to_mat(const double *q, double *R) { pc_quat_to_mat(q, R); }
void pcr_jacobi4(const double *A, double *w, double *V) {
    double B[16];
    memcpy(B, A, sizeof(B));
    pc_jacobi4(B, w, V);
}
/* the ten sums of q q^T, the three of t and the averaged pose of n poses (16 each) */
void pcr_average(const double *poses, const uint32_t *votes, size_t n, double *sums13, double *pose) {
    pc_avg_sums S;
    pc_avg_clear(&S);
    for (size_t i = 0; i < n; ++i) pc_avg_add(&S, poses + 16 * i, votes[i]);
    memcpy(sums13, S.qq, sizeof(double) * 10);
    memcpy(sums13 + 10, S.t, sizeof(double) * 3);
    pc_avg_pose(&S, pose, 0);
}
int pcr_match(const double *a, const double *b, double dist_threshold, double angle_threshold, int level) {
    const uint32_t order[2] = {0, 1};
    double two[32];
    memcpy(two, a, sizeof(double) * 16);
    memcpy(two + 16, b, sizeof(double) * 16);
    Ctx c = {two, order, 0, dist_threshold * dist_threshold, cos(angle_threshold)};
    return match(&c, 0, 1, level);
}
