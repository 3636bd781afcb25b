// test_raycast_mirror.cpp -- the host mirror of the ray cast renderer (misc3d::pose_estimation::RayCastRenderer) over the C
// ABI; built and run by tests/test_gpu_raycast.py.  argv[1]: a blob of width, height (int64), fx, fy, cx, cy (double), the
// number of meshes (int64), then per mesh the numbers of vertices and triangles (int64), the vertices (double), the triangles
// (int32) and the row-major pose (16 doubles).  Prints the getters before a cast, then the maps and the clouds as hex bits.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include <misc3d/pose_estimation/ray_cast_renderer.h>

static uint32_t fbits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}
static uint64_t dbits(double f) {
    uint64_t b;
    std::memcpy(&b, &f, 8);
    return b;
}
static void dump(const char* tag, const misc3d::PointCloud& pc) {
    std::printf("%s %zu %zu\n", tag, pc.points_.size(), pc.normals_.size());
    for (size_t i = 0; i < pc.points_.size(); ++i) {
        for (int c = 0; c < 3; ++c) std::printf("%016" PRIx64 " ", dbits(pc.points_[i][c]));
        for (int c = 0; c < 3; ++c) std::printf("%016" PRIx64 " ", dbits(pc.normals_[i][c]));
        std::printf("\n");
    }
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t wh[2], n_mesh = 0;
    double k[4];
    if (std::fread(wh, 8, 2, f) != 2 || std::fread(k, 8, 4, f) != 4 || std::fread(&n_mesh, 8, 1, f) != 1) return 2;
    std::vector<misc3d::TriangleMesh> meshes(n_mesh);
    std::vector<misc3d::Matrix4d> poses(n_mesh);
    for (int64_t g = 0; g < n_mesh; ++g) {
        int64_t nv = 0, nt = 0;
        if (std::fread(&nv, 8, 1, f) != 1 || std::fread(&nt, 8, 1, f) != 1) return 2;
        meshes[g].vertices_.resize(nv);
        meshes[g].triangles_.resize(nt);
        if (nv && std::fread(meshes[g].vertices_.data(), 24, nv, f) != (size_t)nv) return 2;
        if (nt && std::fread(meshes[g].triangles_.data(), 12, nt, f) != (size_t)nt) return 2;
        if (std::fread(poses[g].data(), 8, 16, f) != 16) return 2;
    }
    std::fclose(f);
    misc3d::pose_estimation::RayCastRenderer renderer((int)wh[0], (int)wh[1], k[0], k[1], k[2], k[3]);
    std::printf("before %zu %zu %zu %zu\n", renderer.GetDepthMap().size(), renderer.GetInstanceMap().size(),
                renderer.GetPointCloud().points_.size(), renderer.GetInstancePointCloud().size());
    std::printf("empty %d\n", (int)renderer.CastRays({}, {}));
    try {
        renderer.CastRays(meshes, {});
    } catch (const std::runtime_error& e) {
        std::printf("%s\n", e.what());
    }
    std::printf("cast %d\n", (int)renderer.CastRays(meshes, poses));
    const std::vector<float> depth = renderer.GetDepthMap();
    const std::vector<uint32_t> inst = renderer.GetInstanceMap(), prim = renderer.GetPrimitiveIds();
    std::printf("maps %zu\n", depth.size());
    for (size_t i = 0; i < depth.size(); ++i) std::printf("%08x %08x %08x\n", fbits(depth[i]), inst[i], prim[i]);
    dump("cloud", renderer.GetPointCloud());
    const std::vector<misc3d::PointCloud> clouds = renderer.GetInstancePointCloud();
    std::printf("instances %zu\n", clouds.size());
    for (const misc3d::PointCloud& pc : clouds) dump("instance", pc);
    return 0;
}
