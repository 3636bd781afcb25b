// m3d_ppf_prepare.hpp -- the host steps of m3d_ppf_prepare_scene (PPFEstimator::PreprocessEstimate, ppf_estimation.cpp:243-278;
// include/misc3d_amd.h): dropping the non-finite points and NormalConsistent.  Plain C++ with no dependency, so that a
// stand-alone program can compile it (tests/cpp/test_ppf_prepare_host.cpp).  Build with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace m3d {

// step 1: the rows of xyz (n x 3) whose three coordinates are finite, order kept; the same rows of normals when given
inline size_t ppf_drop_non_finite(const double* xyz, const double* normals, size_t n, std::vector<double>* pts, std::vector<double>* nrm) {
    pts->clear();
    nrm->clear();
    pts->reserve(3 * n);
    if (normals) nrm->reserve(3 * n);
    for (size_t i = 0; i < n; ++i) {
        const double* p = xyz + 3 * i;
        if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
        pts->insert(pts->end(), p, p + 3);
        if (normals) nrm->insert(nrm->end(), normals + 3 * i, normals + 3 * i + 3);
    }
    return pts->size() / 3;
}

// step 3: NormalConsistent (include/misc3d/utils.h:130-144): towards the origin, then unit length where the length is not zero
inline void ppf_normal_consistent(const double* pts, double* nrm, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const double* p = pts + 3 * i;
        double* v = nrm + 3 * i;
        if ((p[0] * v[0] + p[1] * v[1]) + p[2] * v[2] > 0.0)
            for (int k = 0; k < 3; ++k) v[k] = -v[k];
        const double s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
        if (s > 0.0) {
            const double len = std::sqrt(s);
            for (int k = 0; k < 3; ++k) v[k] = v[k] / len;
        }
    }
}

}  // namespace m3d
