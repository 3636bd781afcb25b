// m3d_ppf.cpp -- the table and the vote of misc3d::pose_estimation::PPFEstimator (src/ppf_estimation.cpp) behind the C ABI:
// m3d_ppf_model_create / _create_edges (CalcHashTable, GenerateModelPCNeighbor), m3d_ppf_vote / _vote_edges (VotingAndGetPose,
// CalcLocalMaximum).  The contract is in include/misc3d_amd.h "PPF voting" and "PPF voting, EdgePoints mode"; the frames
// (CalcTNormal2RegionX) and the pose products are the host's.
// Nothing here depends on M3D_FP_ORDER (every sum is written out).
#include "m3d_driver_internal.hpp"
#include "m3d_ppf.hpp"
#include "m3d_ppf_cluster.hpp"
#include "m3d_radix_sort.hpp"

#include "../../include/misc3d_amd_bench.h"

#include <atomic>

#pragma clang fp contract(off)

using namespace m3d;

namespace {

// m3d_bench_ppf_force
std::atomic<int> g_ppf_force_device{0};
std::atomic<int> g_ppf_max_groups{0};

constexpr size_t kPpfScratchCap = (size_t)256 << 20;        // device scratch of one vote (bytes)
constexpr size_t kPpfFlagBudget = (size_t)160 << 20;        // ... of which the flag arrays
constexpr size_t kPpfAccBudget = (size_t)64 << 20;          // ... and the device-memory accumulators with the row records
constexpr uint64_t kPpfMaxSortPairs = (uint64_t)1 << 28;    // 16 bytes of sort scratch a pair: 4 GiB
constexpr uint32_t kPpfMaxGroups = 256;                     // one workgroup per CU

bool finite3(const double* a, size_t n) {
    for (size_t i = 0; i < 3 * n; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}

// CalcTNormal2RegionX (ppf_estimation.cpp:674-697), rule M3; T row-major 4 x 4
void ppf_frame(const double* p, const double* n, double* T) {
    double u1 = n[2], u2 = -n[1];
    const double norm = std::sqrt(u1 * u1 + u2 * u2);
    if (norm > 1.0e-6) {
        const double inv = 1 / norm;
        u1 *= inv;
        u2 *= inv;
    } else {
        u1 = 1.0;
        u2 = 0.0;
    }
    const double nx = n[0] > 1.0 ? 1.0 : (n[0] < -1.0 ? -1.0 : n[0]);
    const double half = std::acos(nx) / 2;
    const double q0 = std::cos(half), q1 = 0.0, q2 = std::sin(half) * u1, q3 = std::sin(half) * u2;
    double R[9];
    R[0] = 1 - 2 * (q2 * q2 + q3 * q3);
    R[1] = 2 * (q1 * q2 - q0 * q3);
    R[2] = 2 * (q0 * q2 + q1 * q3);
    R[3] = 2 * (q1 * q2 + q0 * q3);
    R[4] = 1 - 2 * (q1 * q1 + q3 * q3);
    R[5] = 2 * (q2 * q3 - q0 * q1);
    R[6] = 2 * (q1 * q3 - q0 * q2);
    R[7] = 2 * (q0 * q1 + q2 * q3);
    R[8] = 1 - 2 * (q1 * q1 + q2 * q2);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[4 * r + c] = R[3 * r + c];
        T[4 * r + 3] = -((R[3 * r] * p[0] + R[3 * r + 1] * p[1]) + R[3 * r + 2] * p[2]);
    }
    T[12] = T[13] = T[14] = 0.0;
    T[15] = 1.0;
}

// C = A B, row-major 4 x 4, every sum ((a0 b0 + a1 b1) + a2 b2) + a3 b3
void mul4(const double* A, const double* B, double* C) {
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            C[4 * r + c] = ((A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c]) + A[4 * r + 3] * B[12 + c];
}

// rule V8: tsg^-1 Rx(alpha) tmg, the inverse being [R^T | -R^T t]
void ppf_pose(const double* tsg, double alpha, const double* tmg, double* out) {
    double inv[16], rx[16], tmp[16];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) inv[4 * r + c] = tsg[4 * c + r];
        inv[4 * r + 3] = -((tsg[r] * tsg[3] + tsg[4 + r] * tsg[7]) + tsg[8 + r] * tsg[11]);
    }
    inv[12] = inv[13] = inv[14] = 0.0;
    inv[15] = 1.0;
    const double ca = std::cos(alpha), sa = std::sin(alpha);
    const double rxv[16] = {1, 0, 0, 0, 0, ca, -sa, 0, 0, sa, ca, 0, 0, 0, 0, 1};
    std::memcpy(rx, rxv, sizeof(rx));
    mul4(inv, rx, tmp);   // (tsg_inv * tr) * tmg, as Eigen evaluates the product
    mul4(tmp, tmg, out);
}

void frame_rows(const double* T, double* rows8) { std::memcpy(rows8, T + 4, sizeof(double) * 8); }

struct VoteBufs {
    DevBuf rpts, rnrm, spts, snrm, ref, sframes, flags, acc, rowinfo, out, small;   // (rpts, rnrm: EdgePoints mode only)
    void release() {
        for (DevBuf* b : {&rpts, &rnrm, &spts, &snrm, &ref, &sframes, &flags, &acc, &rowinfo, &out, &small}) b->release();
    }
};

}  // namespace

struct m3d_ppf_model {
    int device = 0;
    uint32_t n = 0;
    uint32_t n_e = 0;             // the model's edge points (EdgePoints mode), 0 for a SampledPoints model
    double diameter = 0.0, r_min = 0.0, angle_step = 0.0, min_dist_thresh = 0.0, min_angle_thresh = 0.0;
    PpfSizes sizes{};
    PpfTables T{};                // (dist_edge2 points at edge2 below: the host's copy)
    std::vector<double> edge2;
    double centroid[3] = {0, 0, 0};
    std::vector<double> tmg;      // n x 16
    std::vector<double> centred;  // n x 3: the host's copy of pts (the source cloud of m3d_ppf_estimate's refinement)
    uint32_t n_entries = 0, n_neighbors = 0;
    m3d::DevBuf pts, nrm, frames, epts, enrm, d_edge2, cell_off, entries, nbr_off, nbr_idx;   // (epts, enrm: edge models only)
    void release() {
        for (m3d::DevBuf* b : {&pts, &nrm, &frames, &epts, &enrm, &d_edge2, &cell_off, &entries, &nbr_off, &nbr_idx}) b->release();
    }
    bool edges() const { return n_e != 0; }
    PpfModelView view() const {
        PpfModelView v;
        v.T = T;
        v.T.dist_edge2 = d_edge2.as<double>();
        v.n = n;
        v.table_size = (uint32_t)sizes.table_size;
        v.pts = pts.as<double>();
        v.nrm = nrm.as<double>();
        v.frames = frames.as<double>();
        v.same_set = !edges();
        v.epts = edges() ? epts.as<double>() : v.pts;
        v.enrm = edges() ? enrm.as<double>() : v.nrm;
        v.n_e = edges() ? n_e : n;
        v.cell_off = cell_off.as<uint32_t>();
        v.entries = entries.as<uint32_t>();
        v.nbr_off = nbr_off.as<uint32_t>();
        v.nbr_idx = nbr_idx.as<uint32_t>();
        return v;
    }
};

namespace {

int ppf_check_params(const m3d_ppf_params& P, double diameter, double r_min, PpfSizes* sizes) {
    auto pos = [](double v) { return v > 0.0 && std::isfinite(v); };
    if (!pos(diameter) || !pos(r_min)) return fail(M3D_ERR_INVALID_ARG, "ppf: diameter and r_min must be positive and finite");
    if (!pos(P.rel_sample_dist) || !pos(P.angle_step) || !pos(P.min_dist_thresh) || !pos(P.min_angle_thresh))
        return fail(M3D_ERR_INVALID_ARG, "ppf: rel_sample_dist, angle_step, min_dist_thresh and min_angle_thresh must be positive and finite");
    const PpfSizes s = ppf_sizes(diameter, P.rel_sample_dist, P.angle_step);
    if (s.angle_num == 0 || s.alpha_num < 3)
        return fail(M3D_ERR_INVALID_ARG, "ppf: angle_step / rel_sample_dist give fewer than 3 alpha bins or sizes out of range");
    if (s.alpha_num > kPpfMaxAlphaBins)
        return fail(M3D_ERR_INVALID_ARG, "ppf: alpha_model_num = " + std::to_string(s.alpha_num) + " > 64 (angle_step too small)");
    if (s.table_size >= (int64_t)kPpfMaxTableSize) return fail(M3D_ERR_INVALID_ARG, "ppf: hash_table_size must be < 2^24");
    if (!pos(s.dist_step)) return fail(M3D_ERR_INVALID_ARG, "ppf: dist_step is not positive and finite");
    *sizes = s;
    return M3D_OK;
}

// the table and the neighbour lists of a model whose points, normals, frames and edges are on the device
int ppf_build_table(DeviceCtx* ctx, m3d_ppf_model* h) {
    hipStream_t st = ctx->stream;
    const uint32_t n = h->n, table_size = (uint32_t)h->sizes.table_size;
    const uint32_t n_e = h->edges() ? h->n_e : n;
    const uint32_t pairs = n * n_e;   // (<= 2^28: checked by the caller)
    DevBuf keys, k0, v0, k1, v1, counts, scan, total, ncount;
    auto release = [&]() {
        for (DevBuf* b : {&keys, &k0, &v0, &k1, &v1, &counts, &scan, &total, &ncount}) b->release();
    };
    const int rc = [&]() -> int {
        uint32_t tile = 0, blocks = 0;
        voxel_sort_shape(pairs, &tile, &blocks);
        const size_t n_counts = (size_t)kVoxelSortRadix * blocks;
        const uint32_t passes = table_size < (1u << 8) ? 1 : (table_size < (1u << 16) ? 2 : 3);   // (the skipped pairs' key is table_size)
        RESERVE(keys, sizeof(uint32_t) * pairs);
        for (DevBuf* b : {&k0, &v0, &k1, &v1}) RESERVE(*b, sizeof(uint32_t) * pairs);
        RESERVE(counts, sizeof(uint32_t) * n_counts);
        RESERVE(scan, sizeof(uint32_t) * voxel_scan_scratch(std::max<size_t>(n_counts, n + 1)));
        RESERVE(total, 16);
        RESERVE(ncount, sizeof(uint32_t) * (n + 1));
        RESERVE(h->cell_off, sizeof(uint32_t) * ((size_t)table_size + 1));
        RESERVE(h->nbr_off, sizeof(uint32_t) * (n + 1));
        PpfModelView v = h->view();
        launch_ppf_pair_keys(v, keys.as<uint32_t>(), st);
        const uint32_t *sk = nullptr, *sv = nullptr;
        launch_radix_sort_pairs(keys.as<uint32_t>(), nullptr, pairs, passes, k0.as<uint32_t>(), v0.as<uint32_t>(), k1.as<uint32_t>(),
                                v1.as<uint32_t>(), counts.as<uint32_t>(), scan.as<uint32_t>(), total.as<uint32_t>(), &sk, &sv, st);
        launch_ppf_cell_offsets(sk, pairs, table_size, h->cell_off.as<uint32_t>(), st);
        HIPCHK(hipGetLastError());
        // the neighbour lists: counts, their scan, the fill
        const double r = 0.5 * h->r_min, r2 = r * r;
        HIPCHK(hipMemsetAsync(ncount.p, 0, sizeof(uint32_t) * (n + 1), st));
        launch_ppf_nbr_count(v.pts, n, r2, ncount.as<uint32_t>(), st);
        launch_scan_exclusive(ncount.as<uint32_t>(), h->nbr_off.as<uint32_t>(), n + 1, scan.as<uint32_t>(), total.as<uint32_t>(), st);
        HIPCHK(hipGetLastError());
        uint32_t n_entries = 0, n_nbr = 0;
        HIPCHK(hipMemcpyAsync(&n_entries, h->cell_off.as<uint32_t>() + table_size, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&n_nbr, h->nbr_off.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (n_entries > (h->edges() ? pairs : pairs - n) || n_nbr < n || (uint64_t)n_nbr > (uint64_t)n * n)
            return fail(M3D_ERR_INTERNAL, "ppf: the table's totals are out of range (self-check)");
        h->n_entries = n_entries;
        h->n_neighbors = n_nbr;
        RESERVE(h->entries, sizeof(uint32_t) * std::max<size_t>(n_entries, 1));
        RESERVE(h->nbr_idx, sizeof(uint32_t) * n_nbr);
        launch_ppf_entries(sk, sv, n_entries, n_e, table_size, h->entries.as<uint32_t>(), st);
        launch_ppf_nbr_fill(v.pts, n, r2, h->nbr_off.as<uint32_t>(), h->nbr_idx.as<uint32_t>(), st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));   // published to every lane once built
        return M3D_OK;
    }();
    (void)hipStreamSynchronize(st);
    release();
    return rc;
}

// Train (:537-593).  edges == null: rules M1 - M6; else E1 - E5, the referred set being the model's edge points.
m3d_ppf_model* ppf_model_create(const PpfCloud& sample, const PpfCloud* edges, double diameter, double r_min,
                                const m3d_ppf_params* params, int device, int* status) {
    const double *points = sample.pts, *normals = sample.nrm;
    const size_t n = sample.n, n_e = edges ? edges->n : 0;
    if (status) *status = M3D_ERR_INVALID_ARG;
    m3d_ppf_params P;
    m3d_ppf_default_params(&P);
    if (params) P = *params;
    if (!points || !normals) {
        fail(M3D_ERR_INVALID_ARG, "ppf: null points or normals");
        return nullptr;
    }
    if (n < 2 || n > kPpfMaxPoints) {
        fail(M3D_ERR_INVALID_ARG, "ppf: the model must have 2 .. 65535 points, got " + std::to_string(n));
        return nullptr;
    }
    if (edges && (!edges->pts || !edges->nrm)) {
        fail(M3D_ERR_INVALID_ARG, "ppf: null edge points or normals");
        return nullptr;
    }
    if (edges && (n_e < 1 || n_e > kPpfMaxPoints)) {
        fail(M3D_ERR_INVALID_ARG, "ppf: the model must have 1 .. 65535 edge points, got " + std::to_string(n_e));
        return nullptr;
    }
    PpfSizes sizes;
    if (ppf_check_params(P, diameter, r_min, &sizes) != M3D_OK) return nullptr;
    if (!finite3(points, n) || !finite3(normals, n)) {
        fail(M3D_ERR_INVALID_ARG, "ppf: a model point or normal is not finite");
        return nullptr;
    }
    if (edges && (!finite3(edges->pts, n_e) || !finite3(edges->nrm, n_e))) {
        fail(M3D_ERR_INVALID_ARG, "ppf: a model edge point or normal is not finite");
        return nullptr;
    }
    if (status) *status = M3D_ERR_DEVICE;
    if ((uint64_t)n * (edges ? n_e : n) > kPpfMaxSortPairs) {
        fail(M3D_ERR_DEVICE, edges ? "ppf: the table's sort scratch (16 bytes a pair) is capped at 4 GiB: n x n_edge <= 2^28"
                                   : "ppf: the table's sort scratch (16 bytes a pair) is capped at 4 GiB: n <= 16383");
        return nullptr;
    }
    m3d_ppf_model* h = new m3d_ppf_model;
    h->device = device;
    h->n = (uint32_t)n;
    h->n_e = (uint32_t)n_e;
    h->diameter = diameter;
    h->r_min = r_min;
    h->angle_step = P.angle_step;
    h->min_dist_thresh = P.min_dist_thresh;
    h->min_angle_thresh = P.min_angle_thresh;
    h->sizes = sizes;
    ppf_make_tables(sizes, P.angle_step, P.faster_mode != 0, &h->T, &h->edge2);
    // rule M2: the centroid, serially; the centred points; rule M3: the frames
    double c[3] = {0, 0, 0};
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) c[k] += points[3 * i + k];
    for (int k = 0; k < 3; ++k) h->centroid[k] = c[k] / static_cast<double>(n);
    std::vector<double>& centred = h->centred;
    centred.resize(3 * n);
    std::vector<double> rows(8 * n);
    h->tmg.resize(16 * n);
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) centred[3 * i + k] = points[3 * i + k] - h->centroid[k];
        ppf_frame(&centred[3 * i], normals + 3 * i, &h->tmg[16 * i]);
        frame_rows(&h->tmg[16 * i], &rows[8 * i]);
    }
    // rule E1: the edge points are centred by the SAMPLE's centroid
    std::vector<double> ecentred(3 * n_e);
    for (size_t j = 0; j < n_e; ++j)
        for (int k = 0; k < 3; ++k) ecentred[3 * j + k] = edges->pts[3 * j + k] - h->centroid[k];
    if (!finite3(centred.data(), n) || !finite3(ecentred.data(), n_e)) {
        fail(M3D_ERR_INVALID_ARG, "ppf: a centred model point is not finite");
        if (status) *status = M3D_ERR_INVALID_ARG;
        delete h;
        return nullptr;
    }
    int rc = M3D_ERR_DEVICE;
    {
        LaneLock lane(device);
        DeviceCtx* ctx = lane.ctx;
        if (ctx) {
            rc = [&]() -> int {
                HIPCHK(hipSetDevice(ctx->device));
                hipStream_t st = ctx->stream;
                RESERVE(h->pts, sizeof(double) * 3 * n);
                RESERVE(h->nrm, sizeof(double) * 3 * n);
                RESERVE(h->frames, sizeof(double) * 8 * n);
                RESERVE(h->d_edge2, sizeof(double) * h->edge2.size());
                HIPCHK(hipMemcpyAsync(h->pts.p, centred.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, st));
                HIPCHK(hipMemcpyAsync(h->nrm.p, normals, sizeof(double) * 3 * n, hipMemcpyHostToDevice, st));
                HIPCHK(hipMemcpyAsync(h->frames.p, rows.data(), sizeof(double) * 8 * n, hipMemcpyHostToDevice, st));
                HIPCHK(hipMemcpyAsync(h->d_edge2.p, h->edge2.data(), sizeof(double) * h->edge2.size(), hipMemcpyHostToDevice, st));
                if (edges) {
                    RESERVE(h->epts, sizeof(double) * 3 * n_e);
                    RESERVE(h->enrm, sizeof(double) * 3 * n_e);
                    HIPCHK(hipMemcpyAsync(h->epts.p, ecentred.data(), sizeof(double) * 3 * n_e, hipMemcpyHostToDevice, st));
                    HIPCHK(hipMemcpyAsync(h->enrm.p, edges->nrm, sizeof(double) * 3 * n_e, hipMemcpyHostToDevice, st));
                }
                HIPCHK(hipStreamSynchronize(st));
                return ppf_build_table(ctx, h);
            }();
            if (rc != M3D_OK) {
                (void)hipStreamSynchronize(ctx->stream);
                h->release();
            }
        }
    }
    if (rc != M3D_OK) {
        if (status) *status = rc;
        delete h;
        return nullptr;
    }
    if (status) *status = M3D_OK;
    return h;
}

}  // namespace

// what m3d_ppf_cluster.cpp reads of a model (m3d_ppf_cluster.hpp)
m3d::PpfModelHost m3d::ppf_model_host(const m3d_ppf_model* h) {
    PpfModelHost v;
    v.n = h->n;
    v.device = h->device;
    v.diameter = h->diameter;
    v.dist_step = h->sizes.dist_step;
    v.centroid = h->centroid;
    v.centred = h->centred.data();
    v.edges = h->edges();
    return v;
}

// VotingAndGetPose (:399-524), the part that needs no device (m3d_ppf_cluster.hpp).  scene.edges == null (m3d_ppf_vote): the scene
// is scanned and holds the reference points.  Else (m3d_ppf_vote_edges, rules E6 - E8): the reference points are read from the scene
// sample, the scene's edge points are scanned; only the n_ref reference points (gathered) and the edge points go to the device.
int m3d::ppf_check_vote(const m3d_ppf_model* h, const PpfScene& scene, const PpfVoteOut* out, PpfVote* V) {
    const PpfCloud& sc = scene.sample;
    const size_t n_ref = scene.n_ref;
    if (!h) return fail(M3D_ERR_INVALID_ARG, "ppf: null model");
    if ((scene.edges != nullptr) != h->edges())
        return fail(M3D_ERR_INVALID_ARG, scene.edges ? "ppf: the model was trained in SampledPoints mode: vote with m3d_ppf_vote / m3d_ppf_estimate"
                                                     : "ppf: the model was trained in EdgePoints mode: vote with m3d_ppf_vote_edges / m3d_ppf_estimate_edges");
    if (!sc.pts || !sc.nrm || !scene.reference || (out && !out->n_maxima)) return fail(M3D_ERR_INVALID_ARG, "ppf: null argument");
    if (out && out->capacity && (!out->ref_pos || !out->model_index || !out->alpha_index || !out->votes))
        return fail(M3D_ERR_INVALID_ARG, "ppf: null result array");
    if (n_ref == 0) return fail(M3D_ERR_INVALID_ARG, "ppf: no reference points");
    if (sc.n == 0 || sc.n >= ((size_t)1 << 31) || n_ref >= ((size_t)1 << 31)) return fail(M3D_ERR_INVALID_ARG, "ppf: the scene must have 1 .. 2^31 - 1 points");
    if (!finite3(sc.pts, sc.n) || !finite3(sc.nrm, sc.n)) return fail(M3D_ERR_INVALID_ARG, "ppf: a scene point or normal is not finite");
    if (const PpfCloud* e = scene.edges) {
        if (!e->pts || !e->nrm) return fail(M3D_ERR_INVALID_ARG, "ppf: null scene edge points or normals");
        if (e->n == 0 || e->n >= ((size_t)1 << 31)) return fail(M3D_ERR_INVALID_ARG, "ppf: the scene must have 1 .. 2^31 - 1 edge points");
        if (!finite3(e->pts, e->n) || !finite3(e->nrm, e->n)) return fail(M3D_ERR_INVALID_ARG, "ppf: a scene edge point or normal is not finite");
    }
    V->ref.resize(n_ref);
    for (size_t s = 0; s < n_ref; ++s) {
        if (scene.reference[s] >= sc.n) return fail(M3D_ERR_INVALID_ARG, "ppf: a reference index is out of range");
        V->ref[s] = (uint32_t)scene.reference[s];
    }
    V->tsg.resize(16 * n_ref);
    V->rows.resize(8 * n_ref);
    for (size_t s = 0; s < n_ref; ++s) {
        ppf_frame(sc.pts + 3 * (size_t)V->ref[s], sc.nrm + 3 * (size_t)V->ref[s], &V->tsg[16 * s]);
        frame_rows(&V->tsg[16 * s], &V->rows[8 * s]);
    }
    // EdgePoints: the reference points alone, gathered in reference order; position s reads row s
    if (scene.edges) {
        V->rpts.resize(3 * n_ref);
        V->rnrm.resize(3 * n_ref);
        for (size_t s = 0; s < n_ref; ++s) {
            std::memcpy(&V->rpts[3 * s], sc.pts + 3 * (size_t)V->ref[s], sizeof(double) * 3);
            std::memcpy(&V->rnrm[3 * s], sc.nrm + 3 * (size_t)V->ref[s], sizeof(double) * 3);
            V->ref[s] = (uint32_t)s;
        }
    }
    return M3D_OK;
}

// ... and the part on a lane the caller holds: the upload, the kernel, the maxima in rule V8's order
int m3d::ppf_vote_on(DeviceCtx* ctx, const m3d_ppf_model* h, const PpfScene& scene, PpfVote* V) {
    const bool edge = scene.edges != nullptr;
    const PpfCloud& scan = edge ? *scene.edges : scene.sample;   // the cloud the kernel scans
    const size_t m_scan = scan.n, n_ref = scene.n_ref;
    const uint32_t n = h->n;
    const int A = (int)h->sizes.alpha_num;
    const uint32_t table_size = (uint32_t)h->sizes.table_size;
    m3d_ppf_vote_stats& S = V->stats;
    S = m3d_ppf_vote_stats{};
    std::vector<PpfMaximum>& found = V->maxima;
    found.clear();
    const bool lds = ppf_acc_in_lds(n, A) && g_ppf_force_device.load() == 0;
    const size_t acc_words = ppf_acc_words(n, A);
    // the workgroups: what the flag arrays (and, in device memory, the accumulators) leave of the call's scratch
    size_t groups = std::min<size_t>(n_ref, kPpfMaxGroups);
    groups = std::min(groups, std::max<size_t>(1, kPpfFlagBudget / (sizeof(unsigned long long) * table_size)));
    const size_t per_group = sizeof(uint32_t) * ((lds ? 0 : acc_words) + n);
    groups = std::min(groups, std::max<size_t>(1, kPpfAccBudget / per_group));
    if (const int cap = g_ppf_max_groups.load(); cap > 0) groups = std::min<size_t>(groups, (size_t)cap);
    S.path = lds ? M3D_PPF_PATH_LDS : M3D_PPF_PATH_DEVICE;
    S.groups = (uint32_t)groups;

    VoteBufs B;
    const int rc = [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        HIPCHK(hipEventRecord(ctx->ev0, st));
        const size_t fixed = sizeof(double) * (6 * m_scan + (edge ? 14 : 8) * n_ref) + sizeof(uint32_t) * n_ref;
        // room for the maxima of the first launch: the guess m3d_ppf_estimate used to make for its own arrays, and never more
        // than there can be (a maximum is a model row of a reference position)
        size_t out_cap = std::min<size_t>(n_ref * (size_t)n, std::max<size_t>(4096, 4 * n_ref));
        if (fixed + groups * (sizeof(unsigned long long) * table_size + per_group) + sizeof(PpfMaximum) * out_cap > kPpfScratchCap)
            return fail(M3D_ERR_INVALID_ARG, "ppf: the scene and its reference points do not fit the call's 256 MiB of scratch");
        RESERVE(B.spts, sizeof(double) * 3 * m_scan);
        RESERVE(B.snrm, sizeof(double) * 3 * m_scan);
        RESERVE(B.ref, sizeof(uint32_t) * n_ref);
        RESERVE(B.sframes, sizeof(double) * 8 * n_ref);
        RESERVE(B.flags, sizeof(unsigned long long) * table_size * groups);
        if (!lds) RESERVE(B.acc, sizeof(uint32_t) * acc_words * groups);
        RESERVE(B.rowinfo, sizeof(uint32_t) * (size_t)n * groups);
        RESERVE(B.small, 64);
        HIPCHK(hipMemcpyAsync(B.spts.p, scan.pts, sizeof(double) * 3 * m_scan, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(B.snrm.p, scan.nrm, sizeof(double) * 3 * m_scan, hipMemcpyHostToDevice, st));
        if (edge) {
            RESERVE(B.rpts, sizeof(double) * 3 * n_ref);
            RESERVE(B.rnrm, sizeof(double) * 3 * n_ref);
            HIPCHK(hipMemcpyAsync(B.rpts.p, V->rpts.data(), sizeof(double) * 3 * n_ref, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(B.rnrm.p, V->rnrm.data(), sizeof(double) * 3 * n_ref, hipMemcpyHostToDevice, st));
        }
        HIPCHK(hipMemcpyAsync(B.ref.p, V->ref.data(), sizeof(uint32_t) * n_ref, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(B.sframes.p, V->rows.data(), sizeof(double) * 8 * n_ref, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(B.flags.p, 0, sizeof(unsigned long long) * table_size * groups, st));
        PpfVoteArgs a;
        a.M = h->view();
        a.spts = B.spts.as<double>();
        a.snrm = B.snrm.as<double>();
        a.rpts = edge ? B.rpts.as<double>() : a.spts;
        a.rnrm = edge ? B.rnrm.as<double>() : a.snrm;
        a.m = (uint32_t)m_scan;
        a.n_ref = (uint32_t)n_ref;
        a.ref = B.ref.as<uint32_t>();
        a.sframes = B.sframes.as<double>();
        a.r2 = h->r_min * h->r_min;
        a.dist_thresh = h->min_dist_thresh * h->r_min;
        a.cos_thresh = std::cos(h->min_angle_thresh);
        a.gate = (uint32_t)(size_t)((double)(edge ? h->n_e : n) * 0.2);   // (refered_model_num: rules V3 / E7)
        a.acc_words = (uint32_t)acc_words;
        a.flags = B.flags.as<unsigned long long>();
        a.acc = lds ? nullptr : B.acc.as<uint32_t>();
        a.rowinfo = B.rowinfo.as<uint32_t>();
        a.out_count = B.small.as<uint32_t>();
        a.counters = reinterpret_cast<unsigned long long*>(B.small.as<char>() + 8);
        uint64_t head[3] = {0, 0, 0};   // out_count (+ padding), neighbours visited, increments
        for (int attempt = 0; attempt < 2; ++attempt) {
            RESERVE(B.out, sizeof(PpfMaximum) * out_cap);
            a.out = B.out.as<PpfMaximum>();
            a.out_cap = (uint32_t)out_cap;
            HIPCHK(hipMemsetAsync(B.small.p, 0, 24, st));
            HIPCHK(launch_ppf_vote(a, (uint32_t)groups, lds, st));
            S.launches += 1;
            HIPCHK(hipMemcpyAsync(head, B.small.p, 24, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            const size_t count = (uint32_t)head[0];
            if (count <= out_cap) {
                found.resize(count);
                if (count) HIPCHK(hipMemcpy(found.data(), B.out.p, sizeof(PpfMaximum) * count, hipMemcpyDeviceToHost));
                break;
            }
            if (attempt == 1) return fail(M3D_ERR_INTERNAL, "ppf: the second vote found more maxima than the first (self-check)");
            out_cap = count;   // (a maximum is a model row of a reference position: the second run finds the same ones)
        }
        S.neighbours_visited = head[1];
        S.increments = head[2];
        HIPCHK(hipEventRecord(ctx->ev1, st));
        HIPCHK(hipEventSynchronize(ctx->ev1));
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        S.ms_device = ms;
        return M3D_OK;
    }();
    (void)hipStreamSynchronize(ctx->stream);
    B.release();
    if (rc != M3D_OK) return rc;
    // rule V8: ascending (reference position, model index) -- every pair occurs once
    std::sort(found.begin(), found.end(), [](const PpfMaximum& x, const PpfMaximum& y) {
        return x.ref_pos != y.ref_pos ? x.ref_pos < y.ref_pos : x.model_index < y.model_index;
    });
    for (const PpfMaximum& x : found)
        if (x.ref_pos >= n_ref || x.model_index >= n || x.alpha_index >= (uint32_t)A)
            return fail(M3D_ERR_INTERNAL, "ppf: a maximum is out of range (self-check)");
    return M3D_OK;
}

void m3d::ppf_vote_pose(const m3d_ppf_model* h, const PpfVote& V, size_t k, double* pose16) {
    const PpfMaximum& x = V.maxima[k];
    ppf_pose(&V.tsg[16 * (size_t)x.ref_pos], (double)x.alpha_index * h->angle_step, &h->tmg[16 * (size_t)x.model_index], pose16);
}

namespace {

// m3d_ppf_vote / m3d_ppf_vote_edges: check, take a lane, vote on it, then the capacity test and the copy-out
int ppf_vote(const m3d_ppf_model* h, const PpfScene& scene, const PpfVoteOut& out, m3d_ppf_vote_stats* stats) {
    const double t0 = now_ms();
    PpfVote V;
    if (stats) *stats = V.stats;
    if (out.n_maxima) *out.n_maxima = 0;
    if (const int rc = ppf_check_vote(h, scene, &out, &V); rc != M3D_OK) return rc;
    {
        LaneLock lane(h->device);
        if (!lane.ctx) return M3D_ERR_DEVICE;
        if (const int rc = ppf_vote_on(lane.ctx, h, scene, &V); rc != M3D_OK) return rc;
    }
    const size_t found = V.maxima.size();
    *out.n_maxima = found;
    V.stats.ms_total = now_ms() - t0;
    if (stats) *stats = V.stats;
    if (found > out.capacity)
        return fail(M3D_ERR_CAPACITY, "ppf: " + std::to_string(found) + " maxima, the result arrays hold " + std::to_string(out.capacity));
    for (size_t k = 0; k < found; ++k) {
        out.ref_pos[k] = V.maxima[k].ref_pos;
        out.model_index[k] = V.maxima[k].model_index;
        out.alpha_index[k] = V.maxima[k].alpha_index;
        out.votes[k] = V.maxima[k].votes;
        if (out.poses) ppf_vote_pose(h, V, k, out.poses + 16 * k);
    }
    return M3D_OK;
}

}  // namespace

extern "C" {

void m3d_ppf_default_params(m3d_ppf_params* out) {
    if (!out) return;
    out->rel_sample_dist = 0.05;
    out->angle_step = 12.0 / 180.0 * M_PI;
    out->min_dist_thresh = 1.0 / 3.0;
    out->min_angle_thresh = 30.0 / 180.0 * M_PI;
    out->faster_mode = 1;
    out->reserved = 0;
}

m3d_ppf_model* m3d_ppf_model_create(const double* points, const double* normals, size_t n, double diameter, double r_min,
                                    const m3d_ppf_params* params, int device, int* status) {
    return ppf_model_create({points, normals, n}, nullptr, diameter, r_min, params, device, status);
}

m3d_ppf_model* m3d_ppf_model_create_edges(const double* points, const double* normals, size_t n, const double* edge_points,
                                          const double* edge_normals, size_t n_edge, double diameter, double r_min,
                                          const m3d_ppf_params* params, int device, int* status) {
    const PpfCloud edges{edge_points, edge_normals, n_edge};
    return ppf_model_create({points, normals, n}, &edges, diameter, r_min, params, device, status);
}

void m3d_ppf_model_destroy(m3d_ppf_model* h) {
    if (!h) return;
    h->release();
    delete h;
}

size_t m3d_ppf_model_size(const m3d_ppf_model* h) { return h ? h->n : 0; }

size_t m3d_ppf_model_edge_size(const m3d_ppf_model* h) { return h ? h->n_e : 0; }

int m3d_ppf_model_centroid(const m3d_ppf_model* h, double centroid[3]) {
    if (!h || !centroid) return fail(M3D_ERR_INVALID_ARG, "ppf: null argument");
    std::memcpy(centroid, h->centroid, sizeof(double) * 3);
    return M3D_OK;
}

int m3d_ppf_model_table(const m3d_ppf_model* h, m3d_ppf_table_info* info, uint32_t* cell_offsets, uint16_t* entry_i,
                        uint8_t* entry_alpha, uint32_t* nbr_offsets, uint32_t* nbr_indices, double* tmg) {
    if (!h) return fail(M3D_ERR_INVALID_ARG, "ppf: null model");
    if (info) {
        info->table_size = (uint64_t)h->sizes.table_size;
        info->n_entries = h->n_entries;
        info->n_neighbors = h->n_neighbors;
        info->angle_num = (int32_t)h->sizes.angle_num;
        info->alpha_model_num = (int32_t)h->sizes.alpha_num;
        info->dist_num = (int32_t)h->sizes.dist_num;
        info->path = ppf_acc_in_lds(h->n, (int)h->sizes.alpha_num) ? M3D_PPF_PATH_LDS : M3D_PPF_PATH_DEVICE;
    }
    if (tmg) std::memcpy(tmg, h->tmg.data(), sizeof(double) * h->tmg.size());
    if (!cell_offsets && !entry_i && !entry_alpha && !nbr_offsets && !nbr_indices) return M3D_OK;
    LaneLock lane(h->device);
    DeviceCtx* ctx = lane.ctx;
    if (!ctx) return M3D_ERR_DEVICE;
    return [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        std::vector<uint32_t> ent;
        if (cell_offsets)
            HIPCHK(hipMemcpyAsync(cell_offsets, h->cell_off.p, sizeof(uint32_t) * ((size_t)h->sizes.table_size + 1), hipMemcpyDeviceToHost, st));
        if (nbr_offsets) HIPCHK(hipMemcpyAsync(nbr_offsets, h->nbr_off.p, sizeof(uint32_t) * (h->n + 1), hipMemcpyDeviceToHost, st));
        if (nbr_indices) HIPCHK(hipMemcpyAsync(nbr_indices, h->nbr_idx.p, sizeof(uint32_t) * h->n_neighbors, hipMemcpyDeviceToHost, st));
        if ((entry_i || entry_alpha) && h->n_entries) {
            ent.resize(h->n_entries);
            HIPCHK(hipMemcpyAsync(ent.data(), h->entries.p, sizeof(uint32_t) * h->n_entries, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        for (size_t t = 0; t < ent.size(); ++t) {
            if (entry_i) entry_i[t] = (uint16_t)(ent[t] & 0xFFFFu);
            if (entry_alpha) entry_alpha[t] = (uint8_t)(ent[t] >> 16);
        }
        return M3D_OK;
    }();
}

int m3d_ppf_vote(const m3d_ppf_model* h, const double* scene_points, const double* scene_normals, size_t m,
                 const size_t* reference, size_t n_ref, size_t capacity, size_t* n_maxima, uint32_t* ref_pos,
                 uint32_t* model_index, uint32_t* alpha_index, uint32_t* votes, double* poses, m3d_ppf_vote_stats* stats) {
    return ppf_vote(h, {{scene_points, scene_normals, m}, reference, n_ref, nullptr},
                    {capacity, n_maxima, ref_pos, model_index, alpha_index, votes, poses}, stats);
}

int m3d_ppf_vote_edges(const m3d_ppf_model* h, const double* scene_points, const double* scene_normals, size_t m,
                       const size_t* reference, size_t n_ref, const double* scene_edge_points, const double* scene_edge_normals,
                       size_t m_edge, size_t capacity, size_t* n_maxima, uint32_t* ref_pos, uint32_t* model_index,
                       uint32_t* alpha_index, uint32_t* votes, double* poses, m3d_ppf_vote_stats* stats) {
    const PpfCloud edges{scene_edge_points, scene_edge_normals, m_edge};
    return ppf_vote(h, {{scene_points, scene_normals, m}, reference, n_ref, &edges},
                    {capacity, n_maxima, ref_pos, model_index, alpha_index, votes, poses}, stats);
}

// measurement / test hook (include/misc3d_amd_bench.h)
int m3d_bench_ppf_force(int device_memory_path, int max_groups) {
    if (max_groups < 0) return fail(M3D_ERR_INVALID_ARG, "ppf: max_groups must be >= 0");
    g_ppf_force_device.store(device_memory_path != 0);
    g_ppf_max_groups.store(max_groups);
    return M3D_OK;
}

}  // extern "C"
