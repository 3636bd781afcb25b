// m3d_fpfh.cpp -- m3d_estimate_normals, m3d_compute_fpfh and m3d_preprocess_fragment (= PreProcessFragments,
// src/pipeline.cpp:379-401) behind the C ABI: one upload, one k-NN grid, the neighbour searches and everything on top of them
// on the device (m3d_fpfh.hip).  The neighbour lists of a search are KEPT in device memory until the search's consumers have
// run (SPFH needs every list before FPFH starts): 12 bytes per pair, 240 MB for 200 000 points x 100 neighbours.
#include "m3d_driver_internal.hpp"
#include "m3d_fpfh.hpp"
#include "m3d_fpfh_fp.hpp"
#include "m3d_knn_grid.hpp"

#include "../../include/misc3d_amd_bench.h"

#include <optional>

#pragma clang fp contract(off)

using namespace m3d;

namespace {

constexpr size_t kFpfhListCap = (size_t)8 << 30;   // bytes of neighbour lists one search may keep resident

struct SearchArg {
    int search;
    double radius;
    int max_nn;
};

// the argument rules of include/misc3d_amd.h ("Neighbourhood"), decided before any device is touched
int check_search(const char* who, const SearchArg& a) {
    const std::string w(who);
    if (a.search == 1)
        return fail(M3D_ERR_INVALID_ARG, w + ": Radius search (unbounded neighbour lists) is not supported: use "
                                             "KDTreeSearchParamKNN or KDTreeSearchParamHybrid");
    if (a.search != 0 && a.search != 2) return fail(M3D_ERR_INVALID_ARG, w + ": search: 0 = KNN, 2 = Hybrid");
    if (a.max_nn < 1 || a.max_nn > kFpfhMaxNn)
        return fail(M3D_ERR_INVALID_ARG, w + ": max_nn must be in [1, 128], got " + std::to_string(a.max_nn));
    if (a.search == 2 && !(a.radius >= 0.0))
        return fail(M3D_ERR_INVALID_ARG, w + ": the radius of a Hybrid search must be >= 0 and not NaN");
    return M3D_OK;
}

struct Work {
    DevBuf xyz, nrm, q3, l_idx, l_d2, cnt, spfh, out, words, tie_list, tie_packed, tie_rows;
    KnnGrid grid;
    hipEvent_t ev[8] = {};
    int n_ev = 0;
    void release() {
        for (DevBuf* b : {&xyz, &nrm, &q3, &l_idx, &l_d2, &cnt, &spfh, &out, &words, &tie_list, &tie_packed, &tie_rows})
            b->release();
        grid.release();
        for (int k = 0; k < n_ev; ++k) (void)hipEventDestroy(ev[k]);
        n_ev = 0;
    }
};

// what m3d_bench_fpfh_stages takes out of a call, by POINT index; every pointer may be null
struct Capture {
    uint32_t* list_idx;     // n x max_nn; entries at and past cnt: 0xFFFFFFFF
    double* list_d2;        // n x max_nn; entries at and past cnt: +inf
    uint32_t* cnt;          // n
    uint8_t* spfh_count;    // n x 33
    double* spfh_incr;      // n
    uint32_t* tie_points;   // capacity n, ascending
    uint64_t* n_ties;
};

struct Job {
    const double* xyz;
    const double* normals_in;   // may be null
    size_t n;
    bool want_normals;          // estimate them (search sn)
    SearchArg sn;
    int orient;                 // orient the (estimated or given) normals towards cam
    double cam[3];
    bool want_fpfh;
    SearchArg sf;
    double* normals_out;        // may be null
    double* feature_out;        // may be null
    const Capture* cap = nullptr;   // test hook only: filled after the synchronisation that ends the call
};

float ev_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0f;
}

// one search on the lane's stream: lists into W.l_idx / W.l_d2 (nq x kk), counts into W.cnt
int run_search(DeviceCtx* ctx, Work& W, const KnnGridView& v, uint32_t nq, const SearchArg& a, int* kk_out,
               m3d_fpfh_stats& st) {
    const int kk = a.max_nn;
    const size_t pairs = (size_t)nq * (size_t)kk;
    if (pairs * 12 > kFpfhListCap)
        return fail(M3D_ERR_INVALID_ARG, "the neighbour lists of this cloud (12 bytes per pair) exceed 8 GiB: use a smaller max_nn");
    RESERVE(W.l_idx, sizeof(uint32_t) * pairs);
    RESERVE(W.l_d2, sizeof(double) * pairs);
    RESERVE(W.cnt, sizeof(uint32_t) * (size_t)nq);
    unsigned long long* words = W.words.as<unsigned long long>();
    launch_knn_grid(v, W.q3.as<double>(), nq, kk, W.l_d2.as<double>(), W.l_idx.as<uint32_t>(), words, ctx->stream);
    launch_fpfh_count(W.l_d2.as<double>(), nq, kk, a.search == 2, a.radius * a.radius, W.cnt.as<uint32_t>(), words + 1,
                      ctx->stream);
    HIPCHK(hipGetLastError());
    st.launches += 2;
    st.searches += 1;
    *kk_out = kk;
    return M3D_OK;
}

// The SPFH rows of the points the device listed (a pair whose acos comparison is a near tie, m3d_fpfh_fp.hpp): the
// contract's acos is the host libm's, so these rows are evaluated here, by the code the kernel compiles, and put in place
// before FPFH reads them.  Typically a handful of points per 10 000 when the normals were estimated, none when every pair of
// normals is well apart or exactly equal.
int redo_tie_rows(DeviceCtx* ctx, Work& W, const Job& J, const uint32_t* sidx, uint32_t n_ties, int kk, m3d_fpfh_stats& st) {
    hipStream_t s = ctx->stream;
    const size_t rec = 2 + (size_t)kk;
    RESERVE(W.tie_packed, sizeof(uint32_t) * rec * n_ties);
    launch_fpfh_tie_gather(W.tie_list.as<uint32_t>(), n_ties, sidx, W.l_idx.as<uint32_t>(), W.cnt.as<uint32_t>(), kk,
                           W.tie_packed.as<uint32_t>(), s);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> packed(rec * n_ties);
    std::vector<double> nrm(3 * J.n);   // the normals as the device holds them (estimated and / or oriented there)
    HIPCHK(hipMemcpyAsync(packed.data(), W.tie_packed.p, sizeof(uint32_t) * packed.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(nrm.data(), W.nrm.p, sizeof(double) * nrm.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    // rows then points, in one upload: n_ties SpfhRow (48 bytes each) followed by n_ties u32
    std::vector<uint8_t> up(sizeof(SpfhRow) * (size_t)n_ties + sizeof(uint32_t) * (size_t)n_ties, 0);
    SpfhRow* rows = reinterpret_cast<SpfhRow*>(up.data());
    uint32_t* points = reinterpret_cast<uint32_t*>(up.data() + sizeof(SpfhRow) * (size_t)n_ties);
    for (uint32_t e = 0; e < n_ties; ++e) {
        const uint32_t* r = packed.data() + rec * e;
        const uint32_t i = r[0], m = r[1];
        if (i >= J.n || m > (uint32_t)kk) return fail(M3D_ERR_INTERNAL, "fpfh: a tie record is out of range (self-check)");
        uint32_t count[kFpfhDim] = {};
        for (uint32_t k = 1; k < m; ++k) {
            const uint32_t j = r[2 + k];
            if (j >= J.n) return fail(M3D_ERR_INTERNAL, "fpfh: a tie record is out of range (self-check)");
            double f[3];
            int b[3];
            fpfh_pair_features(J.xyz + 3 * (size_t)i, nrm.data() + 3 * (size_t)i, J.xyz + 3 * (size_t)j,
                               nrm.data() + 3 * (size_t)j, f);
            fpfh_bins(f, b);
            for (int t = 0; t < 3; ++t) ++count[b[t]];
        }
        rows[e].incr = fpfh_incr(m);
        for (int t = 0; t < kFpfhDim; ++t) rows[e].count[t] = (uint8_t)count[t];
        points[e] = i;
    }
    RESERVE(W.tie_rows, up.size());
    HIPCHK(hipMemcpyAsync(W.tie_rows.p, up.data(), up.size(), hipMemcpyHostToDevice, s));
    launch_fpfh_tie_scatter(reinterpret_cast<const uint32_t*>(W.tie_rows.as<uint8_t>() + sizeof(SpfhRow) * (size_t)n_ties),
                            W.tie_rows.as<SpfhRow>(), n_ties, W.spfh.as<SpfhRow>(), s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));   // (`up` is pageable and goes out of scope)
    st.launches += 2;
    st.tie_points = n_ties;
    return M3D_OK;
}

// The stages of an FPFH call as the kernels read them, downloaded after the call's last synchronisation and put in point
// order (query t is point sidx[t]).  Only what this call wrote reaches the outputs: list entries below cnt, the SPFH rows of
// finite points (fpfh_spfh_k writes no other; the rest of the downloaded array is not looked at), tie_list below n_ties.
int capture_stages(DeviceCtx* ctx, Work& W, const Job& J, const uint32_t* sidx_dev, uint32_t nq, int kk, uint32_t n_ties) {
    const Capture& c = *J.cap;
    const size_t n = J.n, K = (size_t)J.sf.max_nn;
    if (c.list_idx) std::fill(c.list_idx, c.list_idx + n * K, 0xFFFFFFFFu);
    if (c.list_d2) std::fill(c.list_d2, c.list_d2 + n * K, (double)INFINITY);
    if (c.cnt) std::fill(c.cnt, c.cnt + n, 0u);
    if (c.spfh_count) std::fill(c.spfh_count, c.spfh_count + n * kFpfhDim, (uint8_t)0);
    if (c.spfh_incr) std::fill(c.spfh_incr, c.spfh_incr + n, 0.0);
    if (c.n_ties) *c.n_ties = n_ties;
    if (!nq) return M3D_OK;
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> sidx(nq), idx((size_t)nq * kk), cnt(nq), ties(n_ties);
    std::vector<double> d2((size_t)nq * kk);
    std::vector<SpfhRow> rows(n);
    HIPCHK(hipMemcpyAsync(sidx.data(), sidx_dev, sizeof(uint32_t) * nq, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(idx.data(), W.l_idx.p, sizeof(uint32_t) * idx.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(d2.data(), W.l_d2.p, sizeof(double) * d2.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(cnt.data(), W.cnt.p, sizeof(uint32_t) * nq, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(rows.data(), W.spfh.p, sizeof(SpfhRow) * n, hipMemcpyDeviceToHost, s));
    if (n_ties) HIPCHK(hipMemcpyAsync(ties.data(), W.tie_list.p, sizeof(uint32_t) * n_ties, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (uint32_t t = 0; t < nq; ++t) {
        const size_t i = sidx[t];
        const uint32_t m = cnt[t];
        if (i >= n || m > (uint32_t)kk) return fail(M3D_ERR_INTERNAL, "fpfh stages: a query is out of range (self-check)");
        if (c.cnt) c.cnt[i] = m;
        for (uint32_t k = 0; k < m; ++k) {
            if (c.list_idx) c.list_idx[i * K + k] = idx[(size_t)t * kk + k];
            if (c.list_d2) c.list_d2[i * K + k] = d2[(size_t)t * kk + k];
        }
        if (c.spfh_count) std::memcpy(c.spfh_count + i * kFpfhDim, rows[i].count, kFpfhDim);
        if (c.spfh_incr) c.spfh_incr[i] = rows[i].incr;
    }
    if (c.tie_points) {
        for (uint32_t e = 0; e < n_ties; ++e) {
            if (ties[e] >= nq) return fail(M3D_ERR_INTERNAL, "fpfh stages: a tie entry is out of range (self-check)");
            c.tie_points[e] = sidx[ties[e]];
        }
        std::sort(c.tie_points, c.tie_points + n_ties);
    }
    return M3D_OK;
}

// held != null: on that lane, which the caller holds (m3d_ppf_prepare_model); else the call takes a lane of `device` itself
int run_job(const Job& J, int device, m3d_fpfh_stats* stats, DeviceCtx* held = nullptr) {
    const double t0 = now_ms();
    m3d_fpfh_stats st{};
    const size_t n = J.n;
    std::optional<LaneLock> lane;
    if (!held) lane.emplace(device);
    DeviceCtx* ctx = held ? held : lane->ctx;
    if (!ctx) return M3D_ERR_DEVICE;
    Work W;
    std::vector<uint8_t> finite(n);
    const int rc = [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        for (int k = 0; k < 8; ++k) {
            HIPCHK(hipEventCreate(&W.ev[k]));
            W.n_ev = k + 1;
        }
        size_t nf = 0;
        for (size_t i = 0; i < n; ++i) {
            const double* r = J.xyz + 3 * i;
            finite[i] = std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2]);
            nf += finite[i];
        }
        // ONE grid for the call, of the class of its longest list
        const int kmax = std::max(J.want_normals ? J.sn.max_nn : 1, J.want_fpfh ? J.sf.max_nn : 1);
        const double t_up = now_ms();
        if (nf) {
            if (const int r = knn_build_grid(ctx, J.xyz, n, knn_grid_class(kmax), W.grid); r != M3D_OK) return r;
            if (!W.grid.usable) return fail(M3D_ERR_INVALID_ARG, "the extent of the cloud is not representable in fp64");
        }
        const uint32_t nq = (uint32_t)nf;
        RESERVE(W.xyz, sizeof(double) * 3 * n);
        RESERVE(W.nrm, sizeof(double) * 3 * n);
        RESERVE(W.words, 64);
        HIPCHK(hipMemcpyAsync(W.xyz.p, J.xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
        if (J.normals_in)
            HIPCHK(hipMemcpyAsync(W.nrm.p, J.normals_in, sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(W.words.p, 0, 64, s));
        HIPCHK(hipStreamSynchronize(s));
        st.ms_upload = now_ms() - t_up;
        HIPCHK(hipEventRecord(W.ev[0], s));
        KnnGridView v{};
        if (nq) {
            v = W.grid.view();
            v.data = W.xyz.as<double>();
            RESERVE(W.q3, sizeof(double) * 3 * (size_t)nq);
            launch_fpfh_queries(v.sx, v.sy, v.sz, nq, W.q3.as<double>(), s);
            st.launches += 1;
        }
        int kk = 0;
        uint32_t n_ties = 0;
        // ---- normals
        HIPCHK(hipEventRecord(W.ev[1], s));
        if (J.want_normals && nq)
            if (const int r = run_search(ctx, W, v, nq, J.sn, &kk, st); r != M3D_OK) return r;
        HIPCHK(hipEventRecord(W.ev[2], s));
        if (J.want_normals && nq) {
            launch_fpfh_normals(W.xyz.as<double>(), v.sidx, W.l_idx.as<uint32_t>(), W.cnt.as<uint32_t>(), nq, kk, J.orient,
                                J.cam, W.nrm.as<double>(), s);
            st.launches += 1;
        } else if (!J.want_normals && J.orient) {
            launch_fpfh_orient(W.xyz.as<double>(), (uint32_t)n, J.cam, W.nrm.as<double>(), s);
            st.launches += 1;
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(W.ev[3], s));
        if (J.normals_out)
            HIPCHK(hipMemcpyAsync(J.normals_out, W.nrm.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
        // ---- FPFH
        HIPCHK(hipEventRecord(W.ev[4], s));
        if (J.want_fpfh) {
            RESERVE(W.out, sizeof(double) * kFpfhDim * n);
            HIPCHK(hipMemsetAsync(W.out.p, 0, sizeof(double) * kFpfhDim * n, s));
            if (nq)
                if (const int r = run_search(ctx, W, v, nq, J.sf, &kk, st); r != M3D_OK) return r;
        }
        HIPCHK(hipEventRecord(W.ev[5], s));
        if (J.want_fpfh && nq) {
            RESERVE(W.spfh, sizeof(SpfhRow) * n);
            RESERVE(W.tie_list, sizeof(uint32_t) * (size_t)nq);
            uint32_t* tie_count = reinterpret_cast<uint32_t*>(W.words.as<unsigned long long>() + 2);
            launch_fpfh_spfh(W.xyz.as<double>(), W.nrm.as<double>(), v.sidx, W.l_idx.as<uint32_t>(), W.cnt.as<uint32_t>(), nq,
                             kk, W.spfh.as<SpfhRow>(), W.tie_list.as<uint32_t>(), tie_count, s);
            st.launches += 1;
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&n_ties, tie_count, sizeof(n_ties), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (n_ties > nq) return fail(M3D_ERR_INTERNAL, "fpfh: the tie list overflowed (self-check)");
            if (n_ties)
                if (const int r = redo_tie_rows(ctx, W, J, v.sidx, n_ties, kk, st); r != M3D_OK) return r;
        }
        HIPCHK(hipEventRecord(W.ev[6], s));
        if (J.want_fpfh && nq) {
            launch_fpfh_fpfh(W.spfh.as<SpfhRow>(), v.sidx, W.l_idx.as<uint32_t>(), W.l_d2.as<double>(), W.cnt.as<uint32_t>(),
                             nq, kk, W.out.as<double>(), s);
            st.launches += 1;
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(W.ev[7], s));
        if (J.want_fpfh)
            HIPCHK(hipMemcpyAsync(J.feature_out, W.out.p, sizeof(double) * kFpfhDim * n, hipMemcpyDeviceToHost, s));
        unsigned long long words[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(words, W.words.p, 16, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        st.pairs_seen = words[0];
        st.pairs = words[1];
        st.ms_search = ev_ms(W.ev[1], W.ev[2]) + ev_ms(W.ev[4], W.ev[5]);
        st.ms_normals = ev_ms(W.ev[2], W.ev[3]);
        st.ms_spfh = ev_ms(W.ev[5], W.ev[6]);
        st.ms_fpfh = ev_ms(W.ev[6], W.ev[7]);
        st.ms_device = ev_ms(W.ev[0], W.ev[7]);
        if (J.cap) return capture_stages(ctx, W, J, v.sidx, nq, kk, n_ties);
        return M3D_OK;
    }();
    (void)hipStreamSynchronize(ctx->stream);
    W.release();
    if (rc != M3D_OK) return rc;
    // a point with a non-finite coordinate has no neighbours: the device never visits it
    if (J.normals_out && J.want_normals)
        for (size_t i = 0; i < n; ++i)
            if (!finite[i]) {
                double nn[3] = {0.0, 0.0, 1.0};
                if (J.orient) fpfh_orient(J.xyz + 3 * i, J.cam, nn);
                std::memcpy(J.normals_out + 3 * i, nn, sizeof(nn));
            }
    st.ms_total = now_ms() - t0;
    if (stats) *stats = st;
    return M3D_OK;
}

int check_cloud(const char* who, const double* xyz, size_t n) {
    if (!xyz) return fail(M3D_ERR_INVALID_ARG, std::string(who) + ": null points");
    if (n >= ((size_t)1 << 31)) return fail(M3D_ERR_INVALID_ARG, std::string(who) + ": the number of points must be below 2^31");
    return M3D_OK;
}

}  // namespace

int m3d::estimate_normals_on(DeviceCtx* held, const double* xyz, size_t n, int search, double radius, int max_nn, int orient,
                             const double camera[3], int device, double* normals_out, m3d_normals_stats* stats) {
    if (stats) *stats = m3d_normals_stats{};
    const SearchArg a{search, radius, max_nn};
    if (const int r = check_search("estimate_normals", a); r != M3D_OK) return r;
    if (orient && !camera) return fail(M3D_ERR_INVALID_ARG, "estimate_normals: orient needs a camera location");
    if (n == 0) return M3D_OK;
    if (const int r = check_cloud("estimate_normals", xyz, n); r != M3D_OK) return r;
    if (!normals_out) return fail(M3D_ERR_INVALID_ARG, "estimate_normals: null output");
    Job J{};
    J.xyz = xyz;
    J.n = n;
    J.want_normals = true;
    J.sn = a;
    J.orient = orient ? 1 : 0;
    for (int k = 0; k < 3; ++k) J.cam[k] = orient ? camera[k] : 0.0;
    J.normals_out = normals_out;
    return run_job(J, device, stats, held);
}

extern "C" {

int m3d_estimate_normals(const double* xyz, size_t n, int search, double radius, int max_nn, int orient,
                         const double camera[3], int device, double* normals_out, m3d_normals_stats* stats) {
    return estimate_normals_on(nullptr, xyz, n, search, radius, max_nn, orient, camera, device, normals_out, stats);
}

int m3d_compute_fpfh(const double* xyz, const double* normals, size_t n, int search, double radius, int max_nn, int device,
                     double* feature_out, m3d_fpfh_stats* stats) {
    if (stats) *stats = m3d_fpfh_stats{};
    const SearchArg a{search, radius, max_nn};
    if (const int r = check_search("compute_fpfh", a); r != M3D_OK) return r;
    if (n == 0) return M3D_OK;
    if (!normals) return fail(M3D_ERR_INVALID_ARG, "Failed because input point cloud has no normal.");
    if (const int r = check_cloud("compute_fpfh", xyz, n); r != M3D_OK) return r;
    if (!feature_out) return fail(M3D_ERR_INVALID_ARG, "compute_fpfh: null output");
    Job J{};
    J.xyz = xyz;
    J.normals_in = normals;
    J.n = n;
    J.want_fpfh = true;
    J.sf = a;
    J.feature_out = feature_out;
    return run_job(J, device, stats);
}

int m3d_preprocess_fragment(const double* xyz, const double* normals_in, size_t n, double voxel_size, int device,
                            double* normals_out, double* feature_out, m3d_fpfh_stats* stats) {
    if (stats) *stats = m3d_fpfh_stats{};
    if (!(voxel_size > 0.0) || !std::isfinite(voxel_size))
        return fail(M3D_ERR_INVALID_ARG, "preprocess_fragment: voxel_size must be positive and finite");
    if (n == 0) return M3D_OK;
    if (const int r = check_cloud("preprocess_fragment", xyz, n); r != M3D_OK) return r;
    if (!normals_out || !feature_out) return fail(M3D_ERR_INVALID_ARG, "preprocess_fragment: null output");
    Job J{};
    J.xyz = xyz;
    J.normals_in = normals_in;
    J.n = n;
    J.want_normals = normals_in == nullptr;           // pipeline.cpp:386-389
    J.sn = SearchArg{2, voxel_size * 2.0, 30};
    J.orient = 1;                                     // :390, towards the origin
    J.want_fpfh = true;
    J.sf = SearchArg{2, voxel_size * 5.0, 100};       // :392-394
    J.normals_out = normals_out;
    J.feature_out = feature_out;
    return run_job(J, device, stats);
}

// test hook (include/misc3d_amd_bench.h): the pair features and the bin rule as this library compiles them, on the host
int m3d_bench_fpfh_pair_bins(const double* pairs, size_t m, int32_t* bins, double* features) {
    if ((!pairs || !bins) && m) return fail(M3D_ERR_INVALID_ARG, "null argument");
    for (size_t t = 0; t < m; ++t) {
        const double* p = pairs + 12 * t;
        double f[3];
        int b[3];
        fpfh_pair_features(p, p + 3, p + 6, p + 9, f);
        fpfh_bins(f, b);
        for (int k = 0; k < 3; ++k) {
            bins[3 * t + k] = b[k];
            if (features) features[3 * t + k] = f[k];
        }
    }
    return M3D_OK;
}

// test hook (include/misc3d_amd_bench.h): m3d_compute_fpfh's own job with the stages taken out of it
int m3d_bench_fpfh_stages(const double* xyz, const double* normals, size_t n, int search, double radius, int max_nn, int device,
                          uint32_t* list_idx, double* list_d2, uint32_t* cnt, uint8_t* spfh_count, double* spfh_incr,
                          uint32_t* tie_points, uint64_t* n_ties, double* feature_out, m3d_fpfh_stats* stats) {
    if (stats) *stats = m3d_fpfh_stats{};
    if (n_ties) *n_ties = 0;
    const SearchArg a{search, radius, max_nn};
    if (const int r = check_search("fpfh_stages", a); r != M3D_OK) return r;
    if (n == 0) return M3D_OK;
    if (!normals) return fail(M3D_ERR_INVALID_ARG, "Failed because input point cloud has no normal.");
    if (const int r = check_cloud("fpfh_stages", xyz, n); r != M3D_OK) return r;
    std::vector<double> own;
    if (!feature_out) own.resize(n * (size_t)kFpfhDim);
    const Capture cap{list_idx, list_d2, cnt, spfh_count, spfh_incr, tie_points, n_ties};
    Job J{};
    J.xyz = xyz;
    J.normals_in = normals;
    J.n = n;
    J.want_fpfh = true;
    J.sf = a;
    J.feature_out = feature_out ? feature_out : own.data();
    J.cap = &cap;
    return run_job(J, device, stats);
}

}  // extern "C"
