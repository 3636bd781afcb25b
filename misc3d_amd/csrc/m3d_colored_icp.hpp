// m3d_colored_icp.hpp -- launchers of the colour-gradient kernels (m3d_colored_icp.hip) and the gradient driver
// (m3d_colored_icp.cpp) that m3d_color_gradient and m3d_registration_icp_colored share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "m3d_driver.hpp"

namespace m3d {

// inten[i] = ((c0 + c1) + c2) / 3.0 of colors' row i (rule G3), every row, finite or not
void launch_color_intensity(const double* colors, uint32_t n, double* inten, hipStream_t st);

// color_gradient_k: a lane per query t of the cell-sorted order (point sidx[t]); its list l_idx[t * kk ..] (original
// indices, cnt[t] of them) is walked in list order, rules G2 - G7; three stores into grad's row sidx[t].  Rows of points
// that are no query (a non-finite coordinate) are not written.
void launch_color_gradient(const double* xyz, const double* normals, const double* inten, const uint32_t* sidx,
                           const uint32_t* l_idx, const uint32_t* cnt, uint32_t nq, int kk, double* grad, hipStream_t st);

// The gradients of a target cloud on a lane the caller holds: upload, the k-NN grid, the Hybrid lists (radius, max_nn), the
// intensities and the gradients.  grad (n x 3) and inten (n) stay on the device for the caller, complete in stream order;
// grad_host (may be null) receives the rows, complete when the call returns.
int color_gradient_on(DeviceCtx* ctx, const double* xyz, const double* normals, const double* colors, size_t n, double radius,
                      int max_nn, DevBuf& grad, DevBuf& inten, double* grad_host);

}  // namespace m3d
