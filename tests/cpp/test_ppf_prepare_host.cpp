// test_ppf_prepare_host.cpp -- the two host steps of m3d_ppf_prepare_scene (misc3d_amd/csrc/m3d_ppf_prepare.hpp: dropping the
// non-finite points, NormalConsistent) on hand cases.  No GPU, no library: g++ -O2 -std=c++17 -ffp-contract=off (a stand-alone
// program, so it can also be built with -fsanitize=address,undefined).  Prints "ok" and returns 0, or the first failures and 1.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../misc3d_amd/csrc/m3d_ppf_prepare.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond) && ++g_fail < 20) std::printf("line %d: %s\n", __LINE__, #cond); \
    } while (0)

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // step 1: rows 1 (NaN), 3 (inf) and 4 (-inf in z) go, with their normals; order kept
    const double xyz[6 * 3] = {1, 2, 3, nan, 0, 0, 4, 5, 6, 0, inf, 0, 0, 0, -inf, 7, 8, 9};
    const double nrm[6 * 3] = {0, 0, 1, 1, 0, 0, 0, 1, 0, 1, 1, 1, 2, 2, 2, 3, 0, 4};
    std::vector<double> p, n;
    CHECK(m3d::ppf_drop_non_finite(xyz, nrm, 6, &p, &n) == 3);
    CHECK(p.size() == 9 && n.size() == 9);
    CHECK(p[0] == 1 && p[3] == 4 && p[6] == 7 && p[8] == 9);
    CHECK(n[2] == 1 && n[4] == 1 && n[6] == 3 && n[8] == 4);
    // without normals the second vector stays empty; an empty and an all-NaN cloud give nothing
    CHECK(m3d::ppf_drop_non_finite(xyz, nullptr, 6, &p, &n) == 3 && n.empty());
    CHECK(m3d::ppf_drop_non_finite(xyz, nullptr, 0, &p, &n) == 0 && p.empty());
    CHECK(m3d::ppf_drop_non_finite(xyz + 3, nullptr, 1, &p, &n) == 0);
    // step 3: p . n > 0 negates; then unit length; a zero normal stays; p . n == 0 keeps the sign
    const double pts[5 * 3] = {0, 0, 2, 0, 0, 2, 1, 0, 0, 1, 1, 1, 0, 3, 0};
    double v[5 * 3] = {0, 0, 3, 0, 0, -0.5, 0, 4, 3, 0, 0, 0, -3, 4, 0};
    m3d::ppf_normal_consistent(pts, v, 5);
    CHECK(v[0] == 0 && v[1] == 0 && v[2] == -1);                     // away from the origin: turned, and scaled
    CHECK(v[3] == 0 && v[4] == 0 && v[5] == -1);                     // towards the origin: kept
    CHECK(v[6] == 0 && v[7] == 4.0 / 5.0 && v[8] == 3.0 / 5.0);      // perpendicular: kept
    CHECK(v[9] == 0 && v[10] == 0 && v[11] == 0 && !std::signbit(v[9]));
    CHECK(v[12] == 3.0 / 5.0 && v[13] == -4.0 / 5.0 && v[14] == 0);
    // the division is by sqrt(s), not a multiplication by its reciprocal
    const double q[3] = {-1, -1, -1};
    double w[3] = {0.1, 0.7, 0.3};
    const double s = (0.1 * 0.1 + 0.7 * 0.7) + 0.3 * 0.3;
    m3d::ppf_normal_consistent(q, w, 1);
    CHECK(w[0] == 0.1 / std::sqrt(s) && w[1] == 0.7 / std::sqrt(s) && w[2] == 0.3 / std::sqrt(s));
    if (g_fail) return 1;
    std::printf("ok\n");
    return 0;
}
