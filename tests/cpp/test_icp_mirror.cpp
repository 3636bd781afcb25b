// test_icp_mirror.cpp -- plain g++ user of include/misc3d/reconstruction/multi_scale_icp.h (tests/test_gpu_icp.py):
// reads a blob (n_src, n_dst as uint64; src, dst, dst normals; the initial pose; the voxel size as a double), runs
// RefineFragmentPair and FragmentOdometry with Point2PlaneICP and prints the poses and information matrices as hex words;
// then the errors of a cloud without normals and of ColoredICP.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "misc3d/reconstruction/multi_scale_icp.h"

using namespace misc3d;

static void print_words(const double* v, int n) {
    for (int k = 0; k < n; ++k) {
        uint64_t w;
        std::memcpy(&w, v + k, 8);
        std::printf("%016llx%c", (unsigned long long)w, k + 1 == n ? '\n' : ' ');
    }
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t hdr[2];
    if (std::fread(hdr, 8, 2, f) != 2) return 2;
    std::vector<double> src(3 * hdr[0]), dst(3 * hdr[1]), nrm(3 * hdr[1]);
    Matrix4d init;
    double voxel;
    if (std::fread(src.data(), 8, src.size(), f) != src.size() || std::fread(dst.data(), 8, dst.size(), f) != dst.size() ||
        std::fread(nrm.data(), 8, nrm.size(), f) != nrm.size() || std::fread(init.data(), 8, 16, f) != 16 ||
        std::fread(&voxel, 8, 1, f) != 1)
        return 2;
    std::fclose(f);
    const CloudView s(src.data(), nullptr, hdr[0]), t(dst.data(), nrm.data(), hdr[1]), bare(dst.data(), nullptr, hdr[1]);
    reconstruction::MultiScaleICPOption opt;
    opt.voxel_size = voxel;
    reconstruction::MatchingResult edge;
    edge.transformation_ = init;
    reconstruction::RefineFragmentPair(s, t, edge, opt);
    print_words(edge.transformation_.data(), 16);
    print_words(edge.information_.data(), 36);
    const auto odo = reconstruction::FragmentOdometry(s, t, init, opt);
    print_words(std::get<0>(odo).data(), 16);
    print_words(std::get<1>(odo).data(), 36);
    try {
        reconstruction::FragmentOdometry(s, bare, init, opt);
        std::printf("no error\n");
    } catch (const std::runtime_error& e) {
        std::printf("%s\n", e.what());
    }
    opt.method = reconstruction::LocalRefineMethod::ColoredICP;
    try {
        reconstruction::FragmentOdometry(s, t, init, opt);
        std::printf("no error\n");
    } catch (const std::runtime_error& e) {
        std::printf("%s\n", e.what());
    }
    return 0;
}
