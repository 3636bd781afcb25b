// m3d_host_util.hpp -- the helpers every host translation unit uses around its HIP calls: the two early-return macros, round_up,
// the host clock and the polled end-of-stream wait.  On top of m3d_driver.hpp alone (nothing here depends on M3D_FP_ORDER), so
// the sources outside the driver proper (m3d_registration.cpp, m3d_match.cpp, m3d_global_registration.cpp, m3d_normals.hip)
// take them from here; m3d_driver_internal.hpp includes it for the rest.
#pragma once
#include "m3d_driver.hpp"

#include <chrono>
#include <string>

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return m3d::fail(M3D_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define RESERVE(buf, bytes)                         \
    do {                                            \
        if (!(buf).reserve(bytes)) return M3D_ERR_DEVICE; \
    } while (0)

namespace m3d {

static inline uint32_t round_up(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }
static inline double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// m3d_fit.cpp: the end of the stream's work, polled in page-locked memory
int stream_wait_spin(DeviceCtx* ctx);

}  // namespace m3d
