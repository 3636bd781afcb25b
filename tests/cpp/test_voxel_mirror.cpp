// test_voxel_mirror.cpp -- the host mirror of voxel down-sampling (misc3d::PointCloud::VoxelDownSample,
// preprocessing::VoxelDownSampleMulti, colors_ through SelectByIndex) over the C ABI; built and run by
// tests/test_gpu_voxel.py.  argv[1]: a blob of n, flags (1 normals, 2 colours), then the arrays; argv[2]: the voxel size.
// Prints every output row as the hex bits of its doubles, level by level.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <misc3d/preprocessing/filter.h>

static void dump(const char* tag, const misc3d::PointCloud& pc) {
    std::printf("%s %zu %d %d\n", tag, pc.points_.size(), (int)pc.HasNormals(), (int)pc.HasColors());
    for (size_t j = 0; j < pc.points_.size(); ++j) {
        const misc3d::Vector3d* rows[3] = {&pc.points_[j], pc.HasNormals() ? &pc.normals_[j] : nullptr,
                                           pc.HasColors() ? &pc.colors_[j] : nullptr};
        for (const misc3d::Vector3d* r : rows) {
            if (!r) continue;
            for (int c = 0; c < 3; ++c) {
                uint64_t b;
                std::memcpy(&b, &(*r)[c], 8);
                std::printf("%016" PRIx64 " ", b);
            }
        }
        std::printf("\n");
    }
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n = 0, flags = 0;
    if (std::fread(&n, 8, 1, f) != 1 || std::fread(&flags, 8, 1, f) != 1) return 2;
    misc3d::PointCloud pc;
    pc.points_.resize(n);
    if (std::fread(pc.points_.data(), 24, n, f) != n) return 2;
    if (flags & 1) {
        pc.normals_.resize(n);
        if (std::fread(pc.normals_.data(), 24, n, f) != n) return 2;
    }
    if (flags & 2) {
        pc.colors_.resize(n);
        if (std::fread(pc.colors_.data(), 24, n, f) != n) return 2;
    }
    std::fclose(f);
    const double v = std::atof(argv[2]);
    dump("single", pc.VoxelDownSample(v));
    const std::vector<misc3d::PointCloud> levels = misc3d::preprocessing::VoxelDownSampleMulti(pc, {v, v / 2, v / 4});
    for (const misc3d::PointCloud& l : levels) dump("level", l);
    // colours follow SelectByIndex; a cloud without them behaves as before
    const misc3d::PointCloud sel = pc.SelectByIndex({2, 0});
    std::printf("select %zu %d %d\n", sel.points_.size(), (int)sel.HasNormals(), (int)sel.HasColors());
    if (sel.HasColors()) std::printf("%d\n", (int)(sel.colors_[0] == pc.colors_[2] && sel.colors_[1] == pc.colors_[0]));
    std::printf("empty %zu\n", misc3d::PointCloud().VoxelDownSample(v).points_.size());
    try {
        pc.VoxelDownSample(0.0);
    } catch (const std::runtime_error& e) {
        std::printf("%s\n", e.what());
    }
    return 0;
}
