// ppf_train_host.cpp -- misc3d_amd/csrc/m3d_ppf_train.hpp compiled ALONE with g++ (no HIP, -ffp-contract=off) behind a few C
// symbols, so that tests/test_ppf_train.py can hold the library's host steps of the PPF model preprocessing -- the sampler, the
// signs along a given tree, the box, SampleWithoutDuplicate -- to the restatement without a GPU.
#include "../../misc3d_amd/csrc/m3d_ppf_train.hpp"

extern "C" {

size_t pth_sample(const double* xyz, size_t n, double step, size_t seed, size_t* out, uint64_t* evals) {
    std::vector<size_t> sel;
    m3d::TrainSampleStats st;
    m3d::train_sample(xyz, n, step, seed, &sel, &st);
    std::copy(sel.begin(), sel.end(), out);
    *evals = st.distance_evaluations;
    return sel.size();
}

int pth_tree_signs(const uint32_t* edges, size_t m, const double* normals, size_t n, size_t seed, double* out, int64_t* parent,
                   uint64_t* counts) {
    m3d::OrientCounts c;
    const bool ok = m3d::orient_tree_signs(edges, m, normals, n, seed, out, parent, &c);
    counts[0] = c.component;
    counts[1] = c.flips;
    return ok ? 1 : 0;
}

void pth_box(const double* xyz, size_t n, double* center, double* extent) {
    const m3d::TrainBox b = m3d::train_box(xyz, n);
    for (int k = 0; k < 3; ++k) {
        center[k] = b.center[k];
        extent[k] = b.extent[k];
    }
}

void pth_derive(const double* center, const double* extent, double rel_sample, double rel_dense, double normal_rel, double* out) {
    m3d::TrainBox b;
    for (int k = 0; k < 3; ++k) {
        b.center[k] = center[k];
        b.extent[k] = extent[k];
    }
    const m3d::TrainDerived d = m3d::train_derive(b, rel_sample, rel_dense, normal_rel);
    const double o[8] = {d.diameter, d.r_min, d.dist_step, d.dist_step_dense, d.normal_r, d.view_pt[0], d.view_pt[1], d.view_pt[2]};
    for (int k = 0; k < 8; ++k) out[k] = o[k];
}

size_t pth_seed(const double* xyz, const double* normals, size_t n, const double* view_pt, int invert, int* flips) {
    const size_t s = m3d::train_seed(xyz, n, view_pt);
    *flips = m3d::train_seed_flips(xyz + 3 * s, normals + 3 * s, view_pt, invert != 0) ? 1 : 0;
    return s;
}

void pth_reference_indices(size_t num, size_t sample, uint32_t seed, size_t* out) { m3d::train_reference_indices(num, sample, seed, out); }

}  // extern "C"
