// m3d_knn.cpp -- misc3d::common::KNearestSearch (src/knn.cpp) behind the C ABI: a resident dim x N matrix and exact k
// nearest neighbour queries on it (m3d_knn.hip).  Distances are turned into the returned sqrt on the host, with libm.
#include "m3d_driver_internal.hpp"
#include "m3d_knn_grid.hpp"

#include "../../include/misc3d_amd_bench.h"

#pragma clang fp contract(off)

using namespace m3d;

namespace {

// m3d_bench_knn_force_path: 0 = by shape, else M3D_KNN_PATH_*
std::atomic<int> g_knn_force{0};

constexpr int kKnnMaxDim = 1024;                          // the matcher's cap
constexpr size_t kKnnScratchCap = (size_t)256 << 20;      // device scratch of one call (bytes)
struct KnnBufs {
    DevBuf qT, part_key, part_idx, floor, out_d2, out_idx, q3, seen;
    void release() {
        for (DevBuf* b : {&qT, &part_key, &part_idx, &floor, &out_d2, &out_idx, &q3, &seen}) b->release();
    }
};

}  // namespace

struct m3d_knn {
    int device = 0;
    int dim = 0;
    uint32_t n = 0;
    m3d::DevBuf data;
    std::vector<double> host3;   // dim 3: the rows on the host as well (the grids are built there)
    std::mutex grid_mu;
    KnnGrid grid[kKnnGridClasses];
};

namespace m3d {

constexpr int kKnnGridRowsPerCell[kKnnGridClasses] = {4, 8, 16, 32};   // lists of <= 16, 32, 64, 128 pairs: about kout / 4 rows per cell
constexpr uint64_t kKnnGridMaxCells = (uint64_t)1 << 22;

int knn_grid_class(int kk) { return kk <= 16 ? 0 : kk <= 32 ? 1 : kk <= 64 ? 2 : 3; }

KnnGridView KnnGrid::view() const {
    KnnGridView v;
    v.g = g;
    v.cell_start = cell_start.as<uint32_t>();
    v.sx = sx.as<double>();
    v.sy = sy.as<double>();
    v.sz = sz.as<double>();
    v.sidx = sidx.as<uint32_t>();
    const int na[3] = {g.nx, g.ny, g.nz};
    const double* s = slabs.as<double>();
    for (int a = 0; a < 3; ++a) {
        v.pmax[a] = s;
        v.smin[a] = s + na[a];
        s += 2 * (size_t)na[a];
    }
    v.out_rows = out_rows.as<uint32_t>();
    v.data = nullptr;
    return v;
}
void KnnGrid::release() {
    for (DevBuf* b : {&cell_start, &sx, &sy, &sz, &sidx, &slabs, &out_rows}) b->release();
}

// The density grid of class cls over the finite rows (on the host: a counting sort by cell), uploaded on the caller's
// lane.  Unusable (-> tile path) when there is no finite row or the extent overflows.
int knn_build_grid(DeviceCtx* ctx, const double* p, size_t n, int cls, KnnGrid& G) {
    std::vector<uint32_t> fin, out;
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (size_t i = 0; i < n; ++i) {
        const double* r = p + 3 * i;
        if (!(std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2]))) {
            out.push_back((uint32_t)i);
            continue;
        }
        for (int a = 0; a < 3; ++a) {
            lo[a] = fin.empty() ? r[a] : std::min(lo[a], r[a]);
            hi[a] = fin.empty() ? r[a] : std::max(hi[a], r[a]);
        }
        fin.push_back((uint32_t)i);
    }
    G.built = true;
    G.usable = false;
    double ext[3], emax = 0.0;
    for (int a = 0; a < 3; ++a) {
        ext[a] = hi[a] - lo[a];
        emax = std::max(emax, ext[a]);
    }
    if (fin.empty() || !std::isfinite(emax)) return M3D_OK;
    const uint64_t cap = std::max<uint64_t>(1, std::min<uint64_t>(fin.size() / kKnnGridRowsPerCell[cls], kKnnGridMaxCells));
    auto cells_at = [&](double e) {
        double c = 1.0;
        for (int a = 0; a < 3; ++a) c *= std::floor(ext[a] / e) + 1.0;
        return c;
    };
    double cell = 1.0;
    if (emax > 1e-290) {   // the smallest edge with at most `cap` cells (bisection; cells_at does not increase with the edge)
        double e_lo = emax * 0x1p-23, e_hi = emax * 2.0;
        for (int it = 0; it < 80; ++it) {
            const double mid = 0.5 * (e_lo + e_hi);
            if (cells_at(mid) <= (double)cap)
                e_hi = mid;
            else
                e_lo = mid;
        }
        cell = e_hi;
    }
    const double inv_h = 1.0 / cell;
    int na[3];
    uint64_t ncell = 1;
    for (int a = 0; a < 3; ++a) {
        na[a] = (int)std::min<double>(std::floor(ext[a] * inv_h) + 1.0, (double)kKnnGridMaxCells);
        ncell *= (uint64_t)na[a];
    }
    if (ncell > 2 * kKnnGridMaxCells) return M3D_OK;
    auto cell_of = [&](const double* r, int* c) {
        for (int a = 0; a < 3; ++a) {
            const double v = std::floor((r[a] - lo[a]) * inv_h);
            c[a] = v < 0.0 ? 0 : (v >= (double)na[a] ? na[a] - 1 : (int)v);
        }
        return ((uint64_t)c[2] * (uint64_t)na[1] + (uint64_t)c[1]) * (uint64_t)na[0] + (uint64_t)c[0];
    };
    const size_t nf = fin.size();
    std::vector<uint32_t> start(ncell + 1, 0), cid(nf);
    std::vector<double> slabs(2 * ((size_t)na[0] + na[1] + na[2]));
    double* pm[3];
    double* sm[3];
    {
        double* s = slabs.data();
        for (int a = 0; a < 3; ++a) {
            pm[a] = s;
            sm[a] = s + na[a];
            std::fill(pm[a], pm[a] + na[a], -std::numeric_limits<double>::infinity());
            std::fill(sm[a], sm[a] + na[a], std::numeric_limits<double>::infinity());
            s += 2 * (size_t)na[a];
        }
    }
    for (size_t t = 0; t < nf; ++t) {
        const double* r = p + 3 * (size_t)fin[t];
        int c[3];
        cid[t] = (uint32_t)cell_of(r, c);
        ++start[cid[t] + 1];
        for (int a = 0; a < 3; ++a) {
            pm[a][c[a]] = std::max(pm[a][c[a]], r[a]);
            sm[a][c[a]] = std::min(sm[a][c[a]], r[a]);
        }
    }
    for (int a = 0; a < 3; ++a) {   // per slab -> prefix maximum / suffix minimum
        for (int c = 1; c < na[a]; ++c) pm[a][c] = std::max(pm[a][c], pm[a][c - 1]);
        for (int c = na[a] - 2; c >= 0; --c) sm[a][c] = std::min(sm[a][c], sm[a][c + 1]);
    }
    for (uint64_t c = 0; c < ncell; ++c) start[c + 1] += start[c];
    std::vector<uint32_t> fill(start.begin(), start.end() - 1), sidx(nf);
    std::vector<double> sx(nf), sy(nf), sz(nf);
    for (size_t t = 0; t < nf; ++t) {   // rows in ascending index order within a cell
        const uint32_t at = fill[cid[t]]++;
        const double* r = p + 3 * (size_t)fin[t];
        sx[at] = r[0];
        sy[at] = r[1];
        sz[at] = r[2];
        sidx[at] = fin[t];
    }
    if (out.empty()) out.push_back(0);   // (a word to point at; n_out says how many count)
    hipStream_t s = ctx->stream;
    RESERVE(G.cell_start, sizeof(uint32_t) * start.size());
    RESERVE(G.sx, sizeof(double) * nf);
    RESERVE(G.sy, sizeof(double) * nf);
    RESERVE(G.sz, sizeof(double) * nf);
    RESERVE(G.sidx, sizeof(uint32_t) * nf);
    RESERVE(G.slabs, sizeof(double) * slabs.size());
    RESERVE(G.out_rows, sizeof(uint32_t) * out.size());
    HIPCHK(hipMemcpyAsync(G.cell_start.p, start.data(), sizeof(uint32_t) * start.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(G.sx.p, sx.data(), sizeof(double) * nf, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(G.sy.p, sy.data(), sizeof(double) * nf, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(G.sz.p, sz.data(), sizeof(double) * nf, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(G.sidx.p, sidx.data(), sizeof(uint32_t) * nf, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(G.slabs.p, slabs.data(), sizeof(double) * slabs.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(G.out_rows.p, out.data(), sizeof(uint32_t) * out.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   // published to every lane once built
    G.g.ox = lo[0];
    G.g.oy = lo[1];
    G.g.oz = lo[2];
    G.g.inv_h = inv_h;
    G.g.nx = na[0];
    G.g.ny = na[1];
    G.g.nz = na[2];
    G.g.n_out = (uint32_t)(n - nf);
    G.usable = true;
    return M3D_OK;
}

}  // namespace m3d

namespace {

// What one call needs to put a chunk's results in place.
struct KnnOut {
    size_t stride;
    size_t* indices;
    double* dist;
    double* d2;
    uint32_t n;
};

// Results of rows rows[0 .. mc) (query numbers), columns [col, col + kk), from the host copies of out_idx / out_d2.
int scatter(const KnnOut& o, const uint32_t* rows, uint32_t mc, int kk, size_t col, const uint32_t* idx, const double* dd) {
    for (uint32_t q = 0; q < mc; ++q) {
        const size_t at = (size_t)rows[q] * o.stride + col;
        for (int j = 0; j < kk; ++j) {
            const uint32_t i = idx[(size_t)q * kk + j];
            if (i >= o.n) return fail(M3D_ERR_INTERNAL, "knn: a query's list came back short (self-check)");
            const double v = dd[(size_t)q * kk + j];
            o.indices[at + j] = i;
            o.dist[at + j] = std::sqrt(std::max(v, 0.0));   // (std::max keeps a NaN first argument)
            if (o.d2) o.d2[at + j] = v;
        }
    }
    return M3D_OK;
}

// One chunk of the tile / select path: the mc queries of qT (dim x mc, on the host) against `splits` splits of
// rows_per_split rows, in pages of `page` pairs up to kout; page p > 0 takes only the pairs above the floor (the last
// pair) page p - 1 left.  sink(col, kk, idx, d2) gets the host copies of each page's mc x kk results, raw.
template <class Sink>
int run_tile_chunk(hipStream_t s, KnnBufs& B, const double* data, uint32_t n, int dim, const std::vector<double>& qT,
                   uint32_t mc, int64_t kout, int page, int splits, uint32_t rows_per_split, m3d_knn_stats& st,
                   std::vector<uint32_t>& h_idx, std::vector<double>& h_d2, Sink&& sink) {
    const int kk_max = (int)std::min<int64_t>(page, kout);
    RESERVE(B.qT, sizeof(double) * qT.size());
    RESERVE(B.part_key, sizeof(uint64_t) * (size_t)mc * splits * kk_max);
    RESERVE(B.part_idx, sizeof(uint32_t) * (size_t)mc * splits * kk_max);
    RESERVE(B.floor, sizeof(uint64_t) * 2 * mc);
    RESERVE(B.out_d2, sizeof(double) * (size_t)mc * kk_max);
    RESERVE(B.out_idx, sizeof(uint32_t) * (size_t)mc * kk_max);
    HIPCHK(hipMemcpyAsync(B.qT.p, qT.data(), sizeof(double) * qT.size(), hipMemcpyHostToDevice, s));
    for (int64_t col = 0; col < kout; col += page) {
        const int kk = (int)std::min<int64_t>(page, kout - col);
        launch_knn_tile(data, n, dim, B.qT.as<double>(), mc, kk, splits, rows_per_split,
                        col ? B.floor.as<uint64_t>() : nullptr, B.part_key.as<uint64_t>(), B.part_idx.as<uint32_t>(), s);
        launch_knn_merge(B.part_key.as<uint64_t>(), B.part_idx.as<uint32_t>(), mc, kk, splits,
                         col + kk < kout ? B.floor.as<uint64_t>() : nullptr, B.out_d2.as<double>(),
                         B.out_idx.as<uint32_t>(), s);
        HIPCHK(hipGetLastError());
        st.launches += 2;
        st.pair_dims += (uint64_t)mc * n * (uint64_t)dim;
        h_d2.resize((size_t)mc * kk);
        h_idx.resize((size_t)mc * kk);
        HIPCHK(hipMemcpyAsync(h_d2.data(), B.out_d2.p, sizeof(double) * h_d2.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_idx.data(), B.out_idx.p, sizeof(uint32_t) * h_idx.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (const int r = sink((size_t)col, kk, h_idx.data(), h_d2.data()); r != M3D_OK) return r;
    }
    return M3D_OK;
}

// queries rows[0 .. mc) (row-major, dim each) -> qT (dim x mc)
void transpose_queries(const double* queries, const uint32_t* rows, uint32_t mc, int dim, std::vector<double>& qT) {
    qT.resize((size_t)dim * mc);
    for (uint32_t q = 0; q < mc; ++q) {
        const double* src = queries + (size_t)(rows ? rows[q] : q) * dim;
        for (int k = 0; k < dim; ++k) qT[(size_t)k * mc + q] = src[k];
    }
}

// Tile / select path for the queries rows[0 .. m): chunks of queries, each in pages of `page` pairs.
int run_tile(DeviceCtx* ctx, KnnBufs& B, const m3d_knn* h, const double* queries, const std::vector<uint32_t>& rows,
             int64_t kout, int page, const KnnOut& o, m3d_knn_stats& st) {
    hipStream_t s = ctx->stream;
    const int dim = h->dim;
    const uint32_t n = h->n;
    const size_t m = rows.size();
    const int kk_max = (int)std::min<int64_t>(page, kout);
    auto splits_for = [&](size_t mc) {
        const size_t qblocks = (mc + 63) / 64;
        size_t S = std::min<size_t>(kKnnMaxSplits, (2048 + qblocks - 1) / qblocks);
        S = std::max<size_t>(1, std::min<size_t>(S, (n + 511) / 512));   // at least 512 rows per split
        return S;
    };
    auto bytes_for = [&](size_t mc, size_t S) {
        return mc * ((size_t)dim * 8 + S * (size_t)kk_max * 12 + (size_t)kk_max * 12 + 16);
    };
    size_t mc_max = std::min<size_t>(m, 16384);
    while (mc_max > 1 && bytes_for(mc_max, splits_for(mc_max)) > kKnnScratchCap) mc_max = (mc_max + 1) / 2;
    std::vector<double> qT, h_d2;
    std::vector<uint32_t> h_idx;
    for (size_t c0 = 0; c0 < m; c0 += mc_max) {
        const uint32_t mc = (uint32_t)std::min(mc_max, m - c0);
        const size_t S = splits_for(mc);
        const uint32_t rps = (uint32_t)((n + S - 1) / S);
        const int Sx = (int)((n + rps - 1) / rps);   // no empty split
        transpose_queries(queries, rows.data() + c0, mc, dim, qT);
        const int r = run_tile_chunk(s, B, h->data.as<double>(), n, dim, qT, mc, kout, page, Sx, rps, st, h_idx, h_d2,
                                     [&](size_t col, int kk, const uint32_t* idx, const double* dd) {
                                         return scatter(o, rows.data() + c0, mc, kk, col, idx, dd);
                                     });
        if (r != M3D_OK) return r;
    }
    return M3D_OK;
}

// Grid path for the (finite) queries rows[0 .. m).
int run_grid(DeviceCtx* ctx, KnnBufs& B, const m3d_knn* h, const KnnGrid& G, const double* queries,
             const std::vector<uint32_t>& rows, int kk, const KnnOut& o, m3d_knn_stats& st) {
    hipStream_t s = ctx->stream;
    const size_t m = rows.size();
    const size_t mc_max = 65536;
    KnnGridView v = G.view();
    v.data = h->data.as<double>();
    std::vector<double> q3, h_d2;
    std::vector<uint32_t> h_idx;
    RESERVE(B.seen, 64);
    HIPCHK(hipMemsetAsync(B.seen.p, 0, 8, s));
    for (size_t c0 = 0; c0 < m; c0 += mc_max) {
        const uint32_t mc = (uint32_t)std::min(mc_max, m - c0);
        q3.resize(3 * (size_t)mc);
        for (uint32_t q = 0; q < mc; ++q) std::memcpy(&q3[3 * (size_t)q], queries + 3 * (size_t)rows[c0 + q], 24);
        RESERVE(B.q3, sizeof(double) * q3.size());
        RESERVE(B.out_d2, sizeof(double) * (size_t)mc * kk);
        RESERVE(B.out_idx, sizeof(uint32_t) * (size_t)mc * kk);
        HIPCHK(hipMemcpyAsync(B.q3.p, q3.data(), sizeof(double) * q3.size(), hipMemcpyHostToDevice, s));
        launch_knn_grid(v, B.q3.as<double>(), mc, kk, B.out_d2.as<double>(), B.out_idx.as<uint32_t>(),
                        B.seen.as<unsigned long long>(), s);
        HIPCHK(hipGetLastError());
        st.launches += 1;
        h_d2.resize((size_t)mc * kk);
        h_idx.resize((size_t)mc * kk);
        HIPCHK(hipMemcpyAsync(h_d2.data(), B.out_d2.p, sizeof(double) * h_d2.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_idx.data(), B.out_idx.p, sizeof(uint32_t) * h_idx.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (const int r = scatter(o, rows.data() + c0, mc, kk, 0, h_idx.data(), h_d2.data()); r != M3D_OK) return r;
    }
    unsigned long long seen = 0;
    HIPCHK(hipMemcpy(&seen, B.seen.p, 8, hipMemcpyDeviceToHost));
    st.pair_dims += 3ull * seen;
    return M3D_OK;
}

}  // namespace

extern "C" {

m3d_knn* m3d_knn_create(const double* data, size_t n, int dim, int device, int* status) {
    if (status) *status = M3D_ERR_INVALID_ARG;
    if (dim < 1 || dim > kKnnMaxDim) {
        fail(M3D_ERR_INVALID_ARG, "knn: dim must be in [1, 1024], got " + std::to_string(dim));
        return nullptr;
    }
    if (n == 0 || n >= ((size_t)1 << 31)) {
        fail(M3D_ERR_INVALID_ARG, "knn: the number of rows must be in [1, 2^31)");
        return nullptr;
    }
    if (!data) {
        fail(M3D_ERR_INVALID_ARG, "knn: null data");
        return nullptr;
    }
    if (status) *status = M3D_ERR_DEVICE;
    LaneLock lane(device);
    DeviceCtx* ctx = lane.ctx;
    if (!ctx) return nullptr;
    m3d_knn* h = new m3d_knn;
    h->device = device;
    h->dim = dim;
    h->n = (uint32_t)n;
    const int rc = [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        RESERVE(h->data, sizeof(double) * n * (size_t)dim);
        HIPCHK(hipMemcpyAsync(h->data.p, data, sizeof(double) * n * (size_t)dim, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return M3D_OK;
    }();
    if (rc != M3D_OK) {
        h->data.release();
        delete h;
        return nullptr;
    }
    if (dim == 3) h->host3.assign(data, data + 3 * n);
    if (status) *status = M3D_OK;
    return h;
}

void m3d_knn_destroy(m3d_knn* h) {
    if (!h) return;
    h->data.release();
    for (KnnGrid& G : h->grid) G.release();
    delete h;
}

size_t m3d_knn_size(const m3d_knn* h) { return h ? h->n : 0; }
int m3d_knn_dim(const m3d_knn* h) { return h ? h->dim : 0; }

int m3d_knn_search(const m3d_knn* h, const double* queries, size_t m, int search, int64_t knn, double radius, size_t stride,
                   size_t* indices, double* dist, double* d2, int64_t* counts, m3d_knn_stats* stats) {
    const double t0 = now_ms();
    m3d_knn_stats st{};
    if (stats) *stats = st;
    if (!h) return fail(M3D_ERR_INVALID_ARG, "knn: null index");
    if (search != M3D_KNN_SEARCH_KNN && search != M3D_KNN_SEARCH_HYBRID)
        return fail(M3D_ERR_INVALID_ARG, "knn: search must be KNN (0) or HYBRID (2); radius search is not supported");
    if (knn < 0) return fail(M3D_ERR_INVALID_ARG, "knn: knn must be >= 0");
    const int64_t kout = std::min<int64_t>(knn, (int64_t)h->n);
    if (m == 0) return M3D_OK;
    if (!queries || !counts || (kout > 0 && (!indices || !dist))) return fail(M3D_ERR_INVALID_ARG, "knn: null argument");
    if (stride < (size_t)kout) return fail(M3D_ERR_INVALID_ARG, "knn: stride < min(knn, N)");
    for (size_t q = 0; q < m; ++q)
        for (size_t j = 0; j < stride; ++j) {
            if (indices) indices[q * stride + j] = SIZE_MAX;
            if (dist) dist[q * stride + j] = std::numeric_limits<double>::infinity();
            if (d2) d2[q * stride + j] = std::numeric_limits<double>::infinity();
        }
    if (kout == 0) {
        for (size_t q = 0; q < m; ++q) counts[q] = search == M3D_KNN_SEARCH_KNN ? 0 : -1;
        if (stats) stats->ms_total = now_ms() - t0;
        return M3D_OK;
    }
    if (m >= ((size_t)1 << 32)) return fail(M3D_ERR_INVALID_ARG, "knn: too many queries in one call");
    const int force = g_knn_force.load();
    const bool grid_ok = h->dim == 3 && kout <= kKnnPageMax;
    int path = kout <= kKnnPageMax ? M3D_KNN_PATH_TILE : M3D_KNN_PATH_SELECT;
    if (grid_ok && (force == 0 || force == M3D_KNN_PATH_GRID)) path = M3D_KNN_PATH_GRID;
    if (force == M3D_KNN_PATH_SELECT) path = M3D_KNN_PATH_SELECT;
    const int page = path == M3D_KNN_PATH_SELECT ? (force == M3D_KNN_PATH_SELECT ? 16 : kKnnPageMax) : (int)kout;

    LaneLock lane(h->device);
    DeviceCtx* ctx = lane.ctx;
    if (!ctx) return M3D_ERR_DEVICE;
    KnnBufs B;
    const KnnOut o{stride, indices, dist, d2, h->n};
    const int rc = [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
        std::vector<uint32_t> grid_rows, tile_rows;
        const KnnGrid* G = nullptr;
        if (path == M3D_KNN_PATH_GRID) {
            m3d_knn* hm = const_cast<m3d_knn*>(h);   // the grids are built once, under their mutex
            KnnGrid& g = hm->grid[knn_grid_class((int)kout)];
            {
                std::lock_guard<std::mutex> lock(hm->grid_mu);
                if (!g.built)
                    if (const int r = knn_build_grid(ctx, h->host3.data(), h->n, knn_grid_class((int)kout), g); r != M3D_OK) return r;
            }
            if (g.usable) G = &g;
        }
        if (G) {
            for (size_t q = 0; q < m; ++q) {
                const double* r = queries + 3 * q;
                (std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2]) ? grid_rows : tile_rows)
                    .push_back((uint32_t)q);
            }
        } else {
            if (path == M3D_KNN_PATH_GRID) path = M3D_KNN_PATH_TILE;
            tile_rows.resize(m);
            for (size_t q = 0; q < m; ++q) tile_rows[q] = (uint32_t)q;
        }
        st.path = path;
        if (!grid_rows.empty())
            if (const int r = run_grid(ctx, B, h, *G, queries, grid_rows, (int)kout, o, st); r != M3D_OK) return r;
        if (G) st.tile_queries = tile_rows.size();
        if (!tile_rows.empty())
            if (const int r = run_tile(ctx, B, h, queries, tile_rows, kout, page, o, st); r != M3D_OK) return r;
        HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
        HIPCHK(hipEventSynchronize(ctx->ev1));
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        st.ms_device = ms;
        return M3D_OK;
    }();
    (void)hipStreamSynchronize(ctx->stream);
    B.release();
    if (rc != M3D_OK) return rc;
    for (size_t q = 0; q < m; ++q) {
        if (search == M3D_KNN_SEARCH_KNN) {
            counts[q] = kout;
            continue;
        }
        // knn.cpp:124-138: i = the first position beyond the radius; num = i - 1 (size_t: wraps at i == 0)
        double* dq = dist + q * stride;
        int64_t i = 0;
        while (i < kout && !(dq[i] > radius)) ++i;
        const int64_t num = i - 1;
        counts[q] = num;
        for (int64_t j = std::max<int64_t>(num, 0); j < kout; ++j) {
            indices[q * stride + j] = SIZE_MAX;
            dq[j] = std::numeric_limits<double>::infinity();
            if (d2) d2[q * stride + j] = std::numeric_limits<double>::infinity();
        }
    }
    st.ms_total = now_ms() - t0;
    if (stats) *stats = st;
    return M3D_OK;
}

// measurement / test hook (include/misc3d_amd_bench.h)
int m3d_bench_knn_force_path(int path) {
    if (path < 0 || path > M3D_KNN_PATH_SELECT)
        return fail(M3D_ERR_INVALID_ARG, "path: 0 = by shape, 1 = grid, 2 = tile, 3 = select");
    g_knn_force.store(path);
    return M3D_OK;
}

// test hook (include/misc3d_amd_bench.h): run_tile's chunk with the caller's geometry, results raw
int m3d_bench_knn_tile_merge(const double* data, size_t n, int dim, const double* queries, size_t m, int kk, int pages,
                             int splits, uint32_t rows_per_split, int device, uint32_t* idx_out, uint64_t* d2_bits_out) {
    if (!data || !queries || !idx_out || !d2_bits_out) return fail(M3D_ERR_INVALID_ARG, "knn_tile_merge: null argument");
    if (dim < 1 || dim > kKnnMaxDim) return fail(M3D_ERR_INVALID_ARG, "knn_tile_merge: dim must be in [1, 1024]");
    if (n == 0 || n >= ((size_t)1 << 31) || m == 0 || m >= ((size_t)1 << 31))
        return fail(M3D_ERR_INVALID_ARG, "knn_tile_merge: n and m must be in [1, 2^31)");
    if (kk < 1 || kk > kKnnPageMax) return fail(M3D_ERR_INVALID_ARG, "knn_tile_merge: kk must be in [1, 128]");
    if (pages < 1 || pages > (1 << 20)) return fail(M3D_ERR_INVALID_ARG, "knn_tile_merge: pages must be in [1, 2^20]");
    if (splits < 1 || splits > kKnnMaxSplits) return fail(M3D_ERR_INVALID_ARG, "knn_tile_merge: splits must be in [1, 256]");
    if (rows_per_split < 1) return fail(M3D_ERR_INVALID_ARG, "knn_tile_merge: rows_per_split must be >= 1");
    if ((uint64_t)splits * rows_per_split < n)
        return fail(M3D_ERR_INVALID_ARG, "knn_tile_merge: splits x rows_per_split leaves rows out");
    if (m * ((size_t)dim * 8 + ((size_t)splits + 1) * (size_t)kk * 12 + 16) > kKnnScratchCap)
        return fail(M3D_ERR_INVALID_ARG, "knn_tile_merge: one chunk's scratch is capped at 256 MiB");
    LaneLock lane(device);
    DeviceCtx* ctx = lane.ctx;
    if (!ctx) return M3D_ERR_DEVICE;
    KnnBufs B;
    DevBuf rows;
    const size_t stride = (size_t)pages * kk;
    const int rc = [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        RESERVE(rows, sizeof(double) * n * (size_t)dim);
        HIPCHK(hipMemcpyAsync(rows.p, data, sizeof(double) * n * (size_t)dim, hipMemcpyHostToDevice, s));
        std::vector<double> qT, h_d2;
        std::vector<uint32_t> h_idx;
        m3d_knn_stats st{};
        transpose_queries(queries, nullptr, (uint32_t)m, dim, qT);
        return run_tile_chunk(s, B, rows.as<double>(), (uint32_t)n, dim, qT, (uint32_t)m, (int64_t)stride, kk, splits,
                              rows_per_split, st, h_idx, h_d2, [&](size_t col, int kc, const uint32_t* idx, const double* dd) {
                                  for (size_t q = 0; q < m; ++q) {
                                      std::memcpy(idx_out + q * stride + col, idx + q * kc, sizeof(uint32_t) * kc);
                                      std::memcpy(d2_bits_out + q * stride + col, dd + q * kc, sizeof(double) * kc);
                                  }
                                  return (int)M3D_OK;
                              });
    }();
    (void)hipStreamSynchronize(ctx->stream);
    B.release();
    rows.release();
    return rc;
}

}  // extern "C"
