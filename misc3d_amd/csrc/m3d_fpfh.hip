// m3d_fpfh.hip -- unorganised normal estimation and the FPFH descriptor on gfx950 (include/misc3d_amd.h, "FPFH").
//
// The neighbour lists come from the k-NN grid path (launch_knn_grid, m3d_knn.hip) with the cloud as its own query set and
// stay in device memory for the call.  On top of them:
//   fpfh_count_k    the Hybrid cut: how many leading entries of a list are neighbours
//   fpfh_normals_k  a lane per point: raw sums over the list in list order, J3x3, orientation
//   fpfh_spfh_k     a wavefront per point, lanes over its neighbours: pair features in fp64, the three bins counted with
//                   LDS atomics on integers (order-free), the row stored as counts + the row's one increment (SpfhRow);
//                   a point with a pair whose acos comparison is a near tie is listed: the host redoes its row
//   fpfh_fpfh_k     a wavefront per point, lanes over the 33 bins, neighbours in list order (the contract's accumulation
//                   order): the gather of the neighbours' SPFH rows, 48 bytes each
#include <hip/hip_runtime.h>

#include "m3d_fpfh.hpp"
#include "m3d_fpfh_fp.hpp"
#include "m3d_wave.hpp"

#pragma clang fp contract(off)

namespace m3d {

namespace {

constexpr int kWavesPerBlock = 4;

struct Cam3 {
    double v[3];
};

__global__ __launch_bounds__(256) void fpfh_queries_k(const double* __restrict__ sx, const double* __restrict__ sy,
                                                      const double* __restrict__ sz, uint32_t nq, double* __restrict__ q3) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nq) return;
    q3[3 * (size_t)t] = sx[t];
    q3[3 * (size_t)t + 1] = sy[t];
    q3[3 * (size_t)t + 2] = sz[t];
}

__global__ __launch_bounds__(256) void fpfh_count_k(const double* __restrict__ l_d2, uint32_t nq, int kk, int hybrid,
                                                    double r2, uint32_t* __restrict__ cnt,
                                                    unsigned long long* __restrict__ pairs) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    uint32_t m = 0;
    if (t < nq) {
        const double* d = l_d2 + (size_t)t * kk;
        while (m < (uint32_t)kk) {   // (a NaN -- the empty slot's key -- fails both tests)
            const double v = d[m];
            if (!(v < __builtin_inf()) || (hybrid && !(v < r2))) break;
            ++m;
        }
        cnt[t] = m;
    }
    unsigned long long s = m;
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(pairs, s);
}

__global__ __launch_bounds__(64) void fpfh_normals_k(const double* __restrict__ xyz, const uint32_t* __restrict__ sidx,
                                                     const uint32_t* __restrict__ l_idx, const uint32_t* __restrict__ cnt,
                                                     uint32_t nq, int kk, int orient, Cam3 cam, double* __restrict__ normals) {
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t >= nq) return;
    const uint32_t i = sidx[t], m = cnt[t];
    double n[3] = {0.0, 0.0, 1.0};
    if (m >= 3) {
        double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        const uint32_t* L = l_idx + (size_t)t * kk;
        for (uint32_t k = 0; k < m; ++k) {
            const double* p = xyz + 3 * (size_t)L[k];
            const double x = p[0], y = p[1], z = p[2];
            s[0] += x;
            s[1] += y;
            s[2] += z;
            s[3] += x * x;
            s[4] += x * y;
            s[5] += x * z;
            s[6] += y * y;
            s[7] += y * z;
            s[8] += z * z;
        }
        fpfh_normal_from_sums(s, m, n);
    }
    if (orient) fpfh_orient(xyz + 3 * (size_t)i, cam.v, n);
    normals[3 * (size_t)i] = n[0];
    normals[3 * (size_t)i + 1] = n[1];
    normals[3 * (size_t)i + 2] = n[2];
}

__global__ __launch_bounds__(256) void fpfh_orient_k(const double* __restrict__ xyz, uint32_t n, Cam3 cam,
                                                     double* __restrict__ normals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    double v[3] = {normals[3 * (size_t)i], normals[3 * (size_t)i + 1], normals[3 * (size_t)i + 2]};
    fpfh_orient(xyz + 3 * (size_t)i, cam.v, v);
    normals[3 * (size_t)i] = v[0];
    normals[3 * (size_t)i + 1] = v[1];
    normals[3 * (size_t)i + 2] = v[2];
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void fpfh_spfh_k(const double* __restrict__ xyz,
                                                                   const double* __restrict__ normals,
                                                                   const uint32_t* __restrict__ sidx,
                                                                   const uint32_t* __restrict__ l_idx,
                                                                   const uint32_t* __restrict__ cnt, uint32_t nq, int kk,
                                                                   SpfhRow* __restrict__ spfh,
                                                                   uint32_t* __restrict__ tie_list,
                                                                   uint32_t* __restrict__ tie_count) {
    __shared__ uint32_t bins[kWavesPerBlock][kFpfhDim + 7];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t t = blockIdx.x * (uint32_t)kWavesPerBlock + w;
    const bool live = t < nq;   // (uniform per wavefront; every wavefront reaches the barriers)
    if (lane < kFpfhDim + 7) bins[w][lane] = 0;
    __syncthreads();
    uint32_t i = 0, m = 0;
    bool tie = false;
    if (live) {
        i = sidx[t];
        m = cnt[t];
        const double p1[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
        const double n1[3] = {normals[3 * (size_t)i], normals[3 * (size_t)i + 1], normals[3 * (size_t)i + 2]};
        const uint32_t* L = l_idx + (size_t)t * kk;
        for (uint32_t k = 1 + lane; k < m; k += 64) {   // entry 0 (the point itself) is skipped
            const uint32_t j = L[k];
            const double* p2 = xyz + 3 * (size_t)j;
            const double* n2 = normals + 3 * (size_t)j;
            const double q2[3] = {p2[0], p2[1], p2[2]}, m2[3] = {n2[0], n2[1], n2[2]};
            double f[3];
            int b[3];
            fpfh_pair_features(p1, n1, q2, m2, f, &tie);
            fpfh_bins(f, b);
            atomicAdd(&bins[w][b[0]], 1u);
            atomicAdd(&bins[w][b[1]], 1u);
            atomicAdd(&bins[w][b[2]], 1u);
        }
    }
    __syncthreads();
    const bool any_tie = __any(tie ? 1 : 0) != 0;   // (per wavefront = per point)
    if (live && any_tie && lane == 0) tie_list[atomicAdd(tie_count, 1u)] = t;   // at most one entry per query: < nq
    if (live) {
        SpfhRow* row = spfh + i;
        if (lane < 40) row->count[lane] = lane < kFpfhDim ? (uint8_t)bins[w][lane] : (uint8_t)0;
        if (lane == 0) row->incr = fpfh_incr(m);
    }
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void fpfh_fpfh_k(const SpfhRow* __restrict__ spfh,
                                                                   const uint32_t* __restrict__ sidx,
                                                                   const uint32_t* __restrict__ l_idx,
                                                                   const double* __restrict__ l_d2,
                                                                   const uint32_t* __restrict__ cnt, uint32_t nq, int kk,
                                                                   double* __restrict__ out) {
    __shared__ double accs[kWavesPerBlock][kFpfhDim];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t t = blockIdx.x * (uint32_t)kWavesPerBlock + w;
    const bool live = t < nq;
    const int j = lane < kFpfhDim ? lane : kFpfhDim - 1;   // (lanes >= 33 shadow bin 32 and write nothing)
    uint32_t i = 0, m = 0;
    double acc = 0.0;
    if (live) {
        i = sidx[t];
        m = cnt[t];
        const uint32_t* L = l_idx + (size_t)t * kk;
        const double* D = l_d2 + (size_t)t * kk;
        for (uint32_t k = 1; k < m; ++k) {
            const double d2 = D[k];
            if (d2 == 0.0) continue;
            const SpfhRow* r = spfh + L[k];
            acc += fpfh_weighted(fpfh_spfh_value(r->count[j], r->incr), d2);
        }
    }
    if (lane < kFpfhDim) accs[w][lane] = acc;
    __syncthreads();
    if (live && lane < kFpfhDim) {
        const int g = lane / kFpfhBins;
        double sum = 0.0;
        for (int b = 0; b < kFpfhBins; ++b) sum += accs[w][g * kFpfhBins + b];
        const SpfhRow* own = spfh + i;
        out[(size_t)i * kFpfhDim + lane] = m > 1 ? fpfh_finish(acc, sum, fpfh_spfh_value(own->count[lane], own->incr)) : 0.0;
    }
}

__global__ __launch_bounds__(64) void fpfh_tie_gather_k(const uint32_t* __restrict__ tie_list, uint32_t n_ties,
                                                        const uint32_t* __restrict__ sidx, const uint32_t* __restrict__ l_idx,
                                                        const uint32_t* __restrict__ cnt, int kk, uint32_t* __restrict__ packed) {
    const uint32_t e = blockIdx.x;
    if (e >= n_ties) return;
    const uint32_t t = tie_list[e];
    uint32_t* o = packed + (size_t)e * (2 + kk);
    if (threadIdx.x == 0) {
        o[0] = sidx[t];
        o[1] = cnt[t];
    }
    for (int k = threadIdx.x; k < kk; k += 64) o[2 + k] = l_idx[(size_t)t * kk + k];
}

__global__ __launch_bounds__(64) void fpfh_tie_scatter_k(const uint32_t* __restrict__ points, const SpfhRow* __restrict__ rows,
                                                         uint32_t n_ties, SpfhRow* __restrict__ spfh) {
    const uint32_t e = blockIdx.x * 64u + threadIdx.x;
    if (e >= n_ties) return;
    spfh[points[e]] = rows[e];
}

Cam3 cam_of(const double* c) {
    Cam3 r;
    for (int k = 0; k < 3; ++k) r.v[k] = c ? c[k] : 0.0;
    return r;
}

}  // namespace

void launch_fpfh_queries(const double* sx, const double* sy, const double* sz, uint32_t nq, double* q3, hipStream_t st) {
    if (!nq) return;
    fpfh_queries_k<<<(nq + 255) / 256, 256, 0, st>>>(sx, sy, sz, nq, q3);
}
void launch_fpfh_count(const double* l_d2, uint32_t nq, int kk, int hybrid, double r2, uint32_t* cnt,
                       unsigned long long* pairs, hipStream_t st) {
    if (!nq) return;
    fpfh_count_k<<<(nq + 255) / 256, 256, 0, st>>>(l_d2, nq, kk, hybrid, r2, cnt, pairs);
}
void launch_fpfh_normals(const double* xyz, const uint32_t* sidx, const uint32_t* l_idx, const uint32_t* cnt, uint32_t nq,
                         int kk, int orient, const double* cam3, double* normals, hipStream_t st) {
    if (!nq) return;
    fpfh_normals_k<<<(nq + 63) / 64, 64, 0, st>>>(xyz, sidx, l_idx, cnt, nq, kk, orient, cam_of(cam3), normals);
}
void launch_fpfh_orient(const double* xyz, uint32_t n, const double* cam3, double* normals, hipStream_t st) {
    if (!n) return;
    fpfh_orient_k<<<(n + 255) / 256, 256, 0, st>>>(xyz, n, cam_of(cam3), normals);
}
void launch_fpfh_spfh(const double* xyz, const double* normals, const uint32_t* sidx, const uint32_t* l_idx,
                      const uint32_t* cnt, uint32_t nq, int kk, SpfhRow* spfh, uint32_t* tie_list, uint32_t* tie_count,
                      hipStream_t st) {
    if (!nq) return;
    fpfh_spfh_k<<<(nq + kWavesPerBlock - 1) / kWavesPerBlock, 64 * kWavesPerBlock, 0, st>>>(xyz, normals, sidx, l_idx, cnt, nq,
                                                                                          kk, spfh, tie_list, tie_count);
}
void launch_fpfh_tie_gather(const uint32_t* tie_list, uint32_t n_ties, const uint32_t* sidx, const uint32_t* l_idx,
                            const uint32_t* cnt, int kk, uint32_t* packed, hipStream_t st) {
    if (!n_ties) return;
    fpfh_tie_gather_k<<<n_ties, 64, 0, st>>>(tie_list, n_ties, sidx, l_idx, cnt, kk, packed);
}
void launch_fpfh_tie_scatter(const uint32_t* points, const SpfhRow* rows, uint32_t n_ties, SpfhRow* spfh, hipStream_t st) {
    if (!n_ties) return;
    fpfh_tie_scatter_k<<<(n_ties + 63) / 64, 64, 0, st>>>(points, rows, n_ties, spfh);
}
void launch_fpfh_fpfh(const SpfhRow* spfh, const uint32_t* sidx, const uint32_t* l_idx, const double* l_d2,
                      const uint32_t* cnt, uint32_t nq, int kk, double* out, hipStream_t st) {
    if (!nq) return;
    fpfh_fpfh_k<<<(nq + kWavesPerBlock - 1) / kWavesPerBlock, 64 * kWavesPerBlock, 0, st>>>(spfh, sidx, l_idx, l_d2, cnt, nq, kk,
                                                                                          out);
}

}  // namespace m3d
