// m3d_colored_icp.cpp -- m3d_color_gradient behind the C ABI and the gradient driver m3d_registration_icp_colored shares with it
// (Open3D's InitializePointCloudForColoredICP; the rules G1 - G7 of include/misc3d_amd.h).  One upload, one k-NN grid over the
// target, its Hybrid lists with the target as its own query set (launch_knn_grid + launch_fpfh_count, as the FPFH normals take
// them), then color_gradient_k (m3d_colored_icp.hip).  The lists live in device memory for the call: 12 bytes per pair.
#include "m3d_colored_icp.hpp"
#include "m3d_driver_internal.hpp"
#include "m3d_fpfh.hpp"
#include "m3d_knn_grid.hpp"

using namespace m3d;

namespace {

constexpr size_t kGradientListCap = (size_t)8 << 30;   // bytes of neighbour lists a call may keep resident

struct Work {
    DevBuf xyz, nrm, col, q3, l_idx, l_d2, cnt, words;
    KnnGrid grid;
    void release() {
        for (DevBuf* b : {&xyz, &nrm, &col, &q3, &l_idx, &l_d2, &cnt, &words}) b->release();
        grid.release();
    }
};

}  // namespace

int m3d::color_gradient_on(DeviceCtx* ctx, const double* xyz, const double* normals, const double* colors, size_t n, double radius,
                           int max_nn, DevBuf& grad, DevBuf& inten, double* grad_host) {
    Work W;
    const int rc = [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        size_t nf = 0;
        for (size_t i = 0; i < n; ++i) {
            const double* r = xyz + 3 * i;
            nf += std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2]);
        }
        const int kk = max_nn;
        const size_t pairs = nf * (size_t)kk;
        if (pairs * 12 > kGradientListCap)
            return fail(M3D_ERR_INVALID_ARG, "the neighbour lists of this cloud (12 bytes per pair) exceed 8 GiB: use a smaller max_nn");
        if (nf) {
            if (const int r = knn_build_grid(ctx, xyz, n, knn_grid_class(kk), W.grid); r != M3D_OK) return r;
            if (!W.grid.usable) return fail(M3D_ERR_INVALID_ARG, "the extent of the cloud is not representable in fp64");
        }
        const uint32_t nq = (uint32_t)nf;
        RESERVE(W.xyz, sizeof(double) * 3 * n);
        RESERVE(W.nrm, sizeof(double) * 3 * n);
        RESERVE(W.col, sizeof(double) * 3 * n);
        RESERVE(W.words, 64);
        RESERVE(grad, sizeof(double) * 3 * n);
        RESERVE(inten, sizeof(double) * n);
        HIPCHK(hipMemcpyAsync(W.xyz.p, xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(W.nrm.p, normals, sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(W.col.p, colors, sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(W.words.p, 0, 64, s));
        HIPCHK(hipMemsetAsync(grad.p, 0, sizeof(double) * 3 * n, s));   // (a point that is no query keeps (0, 0, 0): rule G2)
        launch_color_intensity(W.col.as<double>(), (uint32_t)n, inten.as<double>(), s);
        if (nq) {
            KnnGridView v = W.grid.view();
            v.data = W.xyz.as<double>();
            RESERVE(W.q3, sizeof(double) * 3 * (size_t)nq);
            RESERVE(W.l_idx, sizeof(uint32_t) * pairs);
            RESERVE(W.l_d2, sizeof(double) * pairs);
            RESERVE(W.cnt, sizeof(uint32_t) * (size_t)nq);
            unsigned long long* words = W.words.as<unsigned long long>();
            launch_fpfh_queries(v.sx, v.sy, v.sz, nq, W.q3.as<double>(), s);
            launch_knn_grid(v, W.q3.as<double>(), nq, kk, W.l_d2.as<double>(), W.l_idx.as<uint32_t>(), words, s);
            launch_fpfh_count(W.l_d2.as<double>(), nq, kk, 1, radius * radius, W.cnt.as<uint32_t>(), words + 1, s);
            launch_color_gradient(W.xyz.as<double>(), W.nrm.as<double>(), inten.as<double>(), v.sidx, W.l_idx.as<uint32_t>(),
                                  W.cnt.as<uint32_t>(), nq, kk, grad.as<double>(), s);
        }
        HIPCHK(hipGetLastError());
        if (grad_host) HIPCHK(hipMemcpyAsync(grad_host, grad.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
        return M3D_OK;
    }();
    (void)hipStreamSynchronize(ctx->stream);
    W.release();
    return rc;
}

extern "C" int m3d_color_gradient(const double* dst, const double* dst_normals, const double* dst_colors, size_t n, double radius,
                                  int max_nn, int device, double* out_gradient) {
    if (max_nn < 1 || max_nn > 128)
        return fail(M3D_ERR_INVALID_ARG, "color_gradient: max_nn must be in [1, 128], got " + std::to_string(max_nn));
    if (!(radius >= 0.0)) return fail(M3D_ERR_INVALID_ARG, "color_gradient: the radius of a Hybrid search must be >= 0 and not NaN");
    if (n == 0) return M3D_OK;
    if (!dst) return fail(M3D_ERR_INVALID_ARG, "color_gradient: null points");
    if (!dst_normals)
        return fail(M3D_ERR_INVALID_ARG,
                    "TransformationEstimationPointToPlane and TransformationEstimationColoredICP require pre-computed normal "
                    "vectors for target PointCloud.");
    if (!dst_colors) return fail(M3D_ERR_INVALID_ARG, "color_gradient: the target point cloud has no colors.");
    if (n >= ((size_t)1 << 31)) return fail(M3D_ERR_INVALID_ARG, "color_gradient: the number of points must be below 2^31");
    if (!out_gradient) return fail(M3D_ERR_INVALID_ARG, "color_gradient: null output");
    LaneLock lane(device);
    DeviceCtx* ctx = lane.ctx;
    if (!ctx) return M3D_ERR_DEVICE;
    DevBuf grad, inten;
    const int rc = color_gradient_on(ctx, dst, dst_normals, dst_colors, n, radius, max_nn, grad, inten, out_gradient);
    grad.release();
    inten.release();
    return rc;
}
