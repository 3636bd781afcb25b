// m3d_ppf_train.hpp -- the host steps of the PPF model preprocessing (PPFEstimator::PreprocessTrain, ppf_estimation.cpp:206-241
// with :1018-1160; the contract is the block "PPF model preprocessing" of include/misc3d_amd.h): the box and what is derived from
// it (B1, B2), NormalizeNormals (B3), the seed (B4), the signs along the spanning tree the device built (O3, O4), the
// distance-interval sampler (B5) and SampleWithoutDuplicate (C3).  Plain C++ on top of m3d_fp.hpp, m3d_eig3.hpp and
// m3d_mt19937.hpp alone, so that a stand-alone program can compile it with g++.  Build with -ffp-contract=off.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "m3d_eig3.hpp"
#include "m3d_fp.hpp"
#include "m3d_mt19937.hpp"

namespace m3d {

// the squared distance of every search of this file (m3d_proximity_fp.hpp's prox_d2)
inline double train_d2(const double* a, const double* b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// ---- B1: the box.  Mean and covariance as Open3D's ComputeMeanAndCovariance (nine cumulants summed in index order, divided by
// n, cov = E[ab] - E[a] E[b]), the axes from the Jacobi sweeps of m3d_eig3.hpp (column k of V), extent = max - min of
// dot3(axis_k, p - mean), centre = mean + sum_k axis_k (max_k + min_k) / 2.
struct TrainBox {
    double center[3], extent[3];
};
inline TrainBox train_box(const double* xyz, size_t n) {
    double c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < n; ++i) {
        const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        c[0] += x;
        c[1] += y;
        c[2] += z;
        c[3] += x * x;
        c[4] += x * y;
        c[5] += x * z;
        c[6] += y * y;
        c[7] += y * z;
        c[8] += z * z;
    }
    for (int k = 0; k < 9; ++k) c[k] = c[k] / (double)n;
    double A[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    A[0] = c[3] - c[0] * c[0];
    A[4] = c[6] - c[1] * c[1];
    A[8] = c[8] - c[2] * c[2];
    A[1] = A[3] = c[4] - c[0] * c[1];
    A[2] = A[6] = c[5] - c[0] * c[2];
    A[5] = A[7] = c[7] - c[1] * c[2];
    j3x3_jacobi(A, V);
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (size_t i = 0; i < n; ++i) {
        const double dx = xyz[3 * i] - c[0], dy = xyz[3 * i + 1] - c[1], dz = xyz[3 * i + 2] - c[2];
        for (int k = 0; k < 3; ++k) {
            const double v = dot3(V[k], V[3 + k], V[6 + k], dx, dy, dz);
            if (i == 0 || v < lo[k]) lo[k] = v;
            if (i == 0 || v > hi[k]) hi[k] = v;
        }
    }
    TrainBox b;
    double mid[3];
    for (int k = 0; k < 3; ++k) {
        b.extent[k] = hi[k] - lo[k];
        mid[k] = (hi[k] + lo[k]) * 0.5;
    }
    for (int r = 0; r < 3; ++r) b.center[r] = c[r] + ((V[3 * r] * mid[0] + V[3 * r + 1] * mid[1]) + V[3 * r + 2] * mid[2]);
    return b;
}

// ---- B2: what PreprocessTrain derives from the box
struct TrainDerived {
    double diameter, r_min, dist_step, dist_step_dense, normal_r, view_pt[3];
};
inline TrainDerived train_derive(const TrainBox& b, double rel_sample_dist, double rel_dense_sample_dist, double calc_normal_relative) {
    const double* d = b.extent;
    TrainDerived t;
    t.diameter = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    double o[3] = {d[0], d[1], d[2]};
    std::sort(o, o + 3);
    t.r_min = std::sqrt(o[0] * o[0] + o[1] * o[1]);
    t.dist_step = t.diameter * rel_sample_dist;
    t.dist_step_dense = t.diameter * rel_dense_sample_dist;
    t.normal_r = t.diameter * calc_normal_relative;
    t.view_pt[0] = b.center[0];
    t.view_pt[1] = b.center[1];
    t.view_pt[2] = b.center[2] + 2.0 * t.diameter;   // VIEW_POINT_Z_EXTEND
    return t;
}

// ---- B3: NormalizeNormals (a zero normal stays)
inline void train_normalize(double* nrm, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        double* v = nrm + 3 * i;
        const double s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
        if (s > 0.0) {
            const double len = std::sqrt(s);
            for (int k = 0; k < 3; ++k) v[k] = v[k] / len;
        }
    }
}

// ---- B4: the point nearest the view point (lowest index at ties), and whether its normal is flipped
inline size_t train_seed(const double* xyz, size_t n, const double* view_pt) {
    size_t best = 0;
    double bd = 0.0;
    for (size_t i = 0; i < n; ++i) {
        const double d2 = train_d2(view_pt, xyz + 3 * i);
        if (i == 0 || d2 < bd) {
            best = i;
            bd = d2;
        }
    }
    return best;
}
inline bool train_seed_flips(const double* p, const double* nrm, const double* view_pt, bool invert) {
    const bool away = dot3(view_pt[0] - p[0], view_pt[1] - p[1], view_pt[2] - p[2], nrm[0], nrm[1], nrm[2]) < 0.0;
    return away != invert;
}

// ---- O3, O4: the tree edges (m pairs of point indices, any order) -> parent[] and the signed normals.  A breadth-first pass
// from the seed; the forest's other trees are never entered (parent -2, normals unchanged).  -> false: an index out of range
struct OrientCounts {
    uint64_t component = 0, flips = 0;
};
inline bool orient_tree_signs(const uint32_t* edges, size_t m, const double* normals, size_t n, size_t seed, double* out,
                              int64_t* parent, OrientCounts* counts) {
    std::vector<uint32_t> off(n + 1, 0), adj(2 * m);
    for (size_t e = 0; e < 2 * m; ++e) {
        if (edges[e] >= n) return false;
        ++off[edges[e] + 1];
    }
    for (size_t i = 0; i < n; ++i) off[i + 1] += off[i];
    std::vector<uint32_t> cur(off.begin(), off.end() - 1);
    for (size_t e = 0; e < m; ++e) {
        adj[cur[edges[2 * e]]++] = edges[2 * e + 1];
        adj[cur[edges[2 * e + 1]]++] = edges[2 * e];
    }
    std::vector<double> sign(n, 1.0);
    std::vector<uint32_t> queue;
    queue.reserve(n);
    for (size_t i = 0; i < n; ++i) parent[i] = -2;
    for (size_t k = 0; k < 3 * n; ++k) out[k] = normals[k];
    parent[seed] = -1;
    queue.push_back((uint32_t)seed);
    OrientCounts c;
    for (size_t h = 0; h < queue.size(); ++h) {
        const uint32_t p = queue[h];
        const double* np = normals + 3 * p;
        for (uint32_t a = off[p]; a < off[p + 1]; ++a) {
            const uint32_t i = adj[a];
            if (parent[i] != -2) continue;   // (p's own parent)
            parent[i] = p;
            const double* ni = normals + 3 * i;
            if (sign[p] * dot3(ni[0], ni[1], ni[2], np[0], np[1], np[2]) < 0.0) {
                sign[i] = -1.0;
                for (int k = 0; k < 3; ++k) out[3 * i + k] = -ni[k];
                ++c.flips;
            }
            queue.push_back(i);
        }
    }
    c.component = queue.size();
    if (counts) *counts = c;
    return true;
}

// ---- B5: the distance-interval sampler S(step), DownSamplePCNormal as written.  Its radius searches run over a host
// counting-sort grid whose cell edge covers 2 step (1.001 x, doubled while the table would exceed 2^24 cells): a 3x3x3 block
// holds every point with d2 < (2 step)^2, which are then sorted by (d2, index).
struct TrainSampleStats {
    uint64_t distance_evaluations = 0;
};
inline void train_sample(const double* xyz, size_t n, double step, size_t seed, std::vector<size_t>* selected,
                         TrainSampleStats* stats = nullptr) {
    selected->clear();
    if (n == 0) return;
    const double search_r = step * 2;
    const double r2 = search_r * search_r;
    double lo[3], hi[3];
    for (int k = 0; k < 3; ++k) lo[k] = hi[k] = xyz[k];
    for (size_t i = 1; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            lo[k] = std::min(lo[k], xyz[3 * i + k]);
            hi[k] = std::max(hi[k], xyz[3 * i + k]);
        }
    double h = search_r > 0.0 && std::isfinite(search_r * 1.001) ? search_r * 1.001 : 1.0;
    uint64_t dim[3];
    for (;;) {
        bool ok = std::isfinite(h);
        for (int k = 0; k < 3 && ok; ++k) {
            const double cells = std::floor((hi[k] - lo[k]) / h) + 1.0;
            ok = cells < 16777216.0;
            dim[k] = ok ? (uint64_t)cells : 1;
        }
        if (ok && dim[0] * dim[1] * dim[2] <= (UINT64_C(1) << 24)) break;
        if (!std::isfinite(h)) {   // (an extent no finite cell covers: one cell, every pair is tested)
            dim[0] = dim[1] = dim[2] = 1;
            break;
        }
        h = h * 2.0;
    }
    auto cell_of = [&](const double* p, int k) -> uint64_t {
        if (dim[k] == 1) return 0;
        const double f = std::floor((p[k] - lo[k]) / h);
        return f < 0.0 ? 0 : (f >= (double)dim[k] ? dim[k] - 1 : (uint64_t)f);
    };
    const size_t ncell = (size_t)(dim[0] * dim[1] * dim[2]);
    std::vector<uint32_t> start(ncell + 1, 0), order(n), cell(n);
    for (size_t i = 0; i < n; ++i) {
        const double* p = xyz + 3 * i;
        cell[i] = (uint32_t)((cell_of(p, 2) * dim[1] + cell_of(p, 1)) * dim[0] + cell_of(p, 0));
        ++start[cell[i] + 1];
    }
    for (size_t c = 0; c < ncell; ++c) start[c + 1] += start[c];
    {
        std::vector<uint32_t> cur(start.begin(), start.end() - 1);
        for (size_t i = 0; i < n; ++i) order[cur[cell[i]]++] = (uint32_t)i;
    }
    std::vector<char> checked(n, 0);
    std::vector<uint32_t> queue;
    std::vector<std::pair<double, uint32_t>> near;
    queue.push_back((uint32_t)seed);
    uint64_t evals = 0;
    for (size_t qh = 0; qh < queue.size(); ++qh) {
        const uint32_t cur = queue[qh];
        if (checked[cur]) continue;
        checked[cur] = 1;
        selected->push_back(cur);
        const double* p = xyz + 3 * cur;
        const int64_t cx = (int64_t)cell_of(p, 0), cy = (int64_t)cell_of(p, 1), cz = (int64_t)cell_of(p, 2);
        near.clear();
        for (int64_t z = std::max<int64_t>(cz - 1, 0); z <= std::min<int64_t>(cz + 1, (int64_t)dim[2] - 1); ++z)
            for (int64_t y = std::max<int64_t>(cy - 1, 0); y <= std::min<int64_t>(cy + 1, (int64_t)dim[1] - 1); ++y) {
                const int64_t x0 = std::max<int64_t>(cx - 1, 0), x1 = std::min<int64_t>(cx + 1, (int64_t)dim[0] - 1);
                const size_t row = (size_t)((z * (int64_t)dim[1] + y) * (int64_t)dim[0]);
                for (uint32_t s = start[row + x0]; s < start[row + x1 + 1]; ++s) {
                    const uint32_t j = order[s];
                    const double d2 = train_d2(p, xyz + 3 * j);
                    ++evals;
                    if (d2 < r2) near.emplace_back(d2, j);
                }
            }
        std::sort(near.begin(), near.end());
        for (const auto& nb : near) {
            if (checked[nb.second]) continue;
            if (std::sqrt(nb.first) < step) checked[nb.second] = 1;
            else queue.push_back(nb.second);
        }
    }
    if (stats) stats->distance_evaluations = evals;
}

// ---- C3: RandomSampler<size_t>(num).SampleWithoutDuplicate(sample) on std::mt19937(seed) (utils.h:101-116); its
// swap(indices[i], indices[rng() % num]) is not Fisher-Yates and is kept as written.  sample <= num, 0 < num < 2^32
inline void train_reference_indices(size_t num, size_t sample, uint32_t seed, size_t* out) {
    std::vector<size_t> indices(num);
    for (size_t i = 0; i < num; ++i) indices[i] = i;
    Mt19937Mod rng;
    rng.seed(seed);
    rng.set_modulus((uint32_t)num);
    for (size_t i = 0; i < sample; ++i) std::swap(indices[i], indices[rng.next()]);
    for (size_t i = 0; i < sample; ++i) out[i] = indices[i];
}

}  // namespace m3d
