// m3d_colored_icp.hip -- the per-point colour gradient of coloured ICP on gfx950 (include/misc3d_amd.h, m3d_color_gradient:
// Open3D's InitializePointCloudForColoredICP).  The neighbour lists are the Hybrid lists of the k-NN grid path
// (launch_knn_grid + launch_fpfh_count) with the target as its own query set; on top of them:
//   color_intensity_k   I = ((c0 + c1) + c2) / 3.0, once per point
//   color_gradient_k    a lane per point: the rows of rules G4 and G5 in list order, the serial sums of G6 written out, the
//                       3 x 3 LDLT of m3d_icp_fp.hpp (the text the host compiles), three stores
// Every sum here is written out with its association; nothing goes through m3d_fp.hpp.
#include <hip/hip_runtime.h>

#include "m3d_colored_icp.hpp"
#include "m3d_icp_fp.hpp"

#pragma clang fp contract(off)

namespace m3d {

namespace {

__global__ __launch_bounds__(256) void color_intensity_k(const double* __restrict__ colors, uint32_t n,
                                                         double* __restrict__ inten) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const double* c = colors + 3 * (size_t)i;
    inten[i] = ((c[0] + c[1]) + c[2]) / 3.0;
}

__global__ __launch_bounds__(64) void color_gradient_k(const double* __restrict__ xyz, const double* __restrict__ normals,
                                                       const double* __restrict__ inten, const uint32_t* __restrict__ sidx,
                                                       const uint32_t* __restrict__ l_idx, const uint32_t* __restrict__ cnt,
                                                       uint32_t nq, int kk, double* __restrict__ grad) {
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t >= nq) return;
    const uint32_t i = sidx[t], nn = cnt[t];
    double g[3] = {0.0, 0.0, 0.0};
    if (nn >= 4) {
        const double v0 = xyz[3 * (size_t)i], v1 = xyz[3 * (size_t)i + 1], v2 = xyz[3 * (size_t)i + 2];
        const double n0 = normals[3 * (size_t)i], n1 = normals[3 * (size_t)i + 1], n2 = normals[3 * (size_t)i + 2];
        const double ik = inten[i];
        double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        const uint32_t* L = l_idx + (size_t)t * kk;
        for (uint32_t k = 1; k < nn; ++k) {   // entry 0 is skipped whatever it is
            const uint32_t j = L[k];
            const double* p = xyz + 3 * (size_t)j;
            const double p0 = p[0], p1 = p[1], p2 = p[2];
            const double s = ((p0 - v0) * n0 + (p1 - v1) * n1) + (p2 - v2) * n2;
            const double r0 = (p0 - s * n0) - v0, r1 = (p1 - s * n1) - v1, r2 = (p2 - s * n2) - v2;
            const double bi = inten[j] - ik;
            a00 += r0 * r0;
            a01 += r0 * r1;
            a02 += r0 * r2;
            a11 += r1 * r1;
            a12 += r1 * r2;
            a22 += r2 * r2;
            b0 += r0 * bi;
            b1 += r1 * bi;
            b2 += r2 * bi;
        }
        {   // the constraint row: (nn - 1) n, right-hand side 0
            const double w = (double)(nn - 1);
            const double r0 = w * n0, r1 = w * n1, r2 = w * n2;
            a00 += r0 * r0;
            a01 += r0 * r1;
            a02 += r0 * r2;
            a11 += r1 * r1;
            a12 += r1 * r2;
            a22 += r2 * r2;
            b0 += r0 * 0.0;
            b1 += r1 * 0.0;
            b2 += r2 * 0.0;
        }
        const double A[9] = {a00, a01, a02, a01, a11, a12, a02, a12, a22};
        const double b[3] = {b0, b1, b2};
        icp_ldlt_solve3(A, b, g);
    }
    grad[3 * (size_t)i] = g[0];
    grad[3 * (size_t)i + 1] = g[1];
    grad[3 * (size_t)i + 2] = g[2];
}

}  // namespace

void launch_color_intensity(const double* colors, uint32_t n, double* inten, hipStream_t st) {
    if (!n) return;
    color_intensity_k<<<(n + 255) / 256, 256, 0, st>>>(colors, n, inten);
}
void launch_color_gradient(const double* xyz, const double* normals, const double* inten, const uint32_t* sidx,
                           const uint32_t* l_idx, const uint32_t* cnt, uint32_t nq, int kk, double* grad, hipStream_t st) {
    if (!nq) return;
    color_gradient_k<<<(nq + 63) / 64, 64, 0, st>>>(xyz, normals, inten, sidx, l_idx, cnt, nq, kk, grad);
}

}  // namespace m3d
