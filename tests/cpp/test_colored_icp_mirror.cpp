// test_colored_icp_mirror.cpp -- plain g++ user of include/misc3d/reconstruction/multi_scale_icp.h
// (tests/test_gpu_colored_icp.py): reads a blob (n_src, n_dst as uint64; src, src colours, dst, dst normals, dst colours; the
// initial pose; the voxel size as a double), runs RefineFragmentPair with ColoredICP on views that carry colours and prints the
// pose and the information matrix as hex words; then the error of the same call on views without colours.
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
    std::vector<double> src(3 * hdr[0]), scol(3 * hdr[0]), dst(3 * hdr[1]), nrm(3 * hdr[1]), dcol(3 * hdr[1]);
    Matrix4d init;
    double voxel;
    for (std::vector<double>* v : {&src, &scol, &dst, &nrm, &dcol})
        if (std::fread(v->data(), 8, v->size(), f) != v->size()) return 2;
    if (std::fread(init.data(), 8, 16, f) != 16 || std::fread(&voxel, 8, 1, f) != 1) return 2;
    std::fclose(f);
    const CloudView s(src.data(), nullptr, scol.data(), hdr[0]), t(dst.data(), nrm.data(), dcol.data(), hdr[1]);
    const CloudView bare(dst.data(), nrm.data(), hdr[1]);
    reconstruction::MultiScaleICPOption opt;
    opt.voxel_size = voxel;
    opt.method = reconstruction::LocalRefineMethod::ColoredICP;
    reconstruction::MatchingResult edge;
    edge.transformation_ = init;
    reconstruction::RefineFragmentPair(s, t, edge, opt);
    print_words(edge.transformation_.data(), 16);
    print_words(edge.information_.data(), 36);
    try {
        edge.transformation_ = init;
        reconstruction::RefineFragmentPair(s, bare, edge, opt);
        std::printf("no error\n");
    } catch (const std::runtime_error& e) {
        std::printf("%s\n", e.what());
    }
    return 0;
}
