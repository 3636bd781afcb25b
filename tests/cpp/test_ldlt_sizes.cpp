// test_ldlt_sizes.cpp -- host-side check of the pivoted LDL^T of misc3d_amd/csrc/m3d_icp_fp.hpp at both sizes (the text the
// library and color_gradient_k compile): no GPU, no library.
//   six             digests (FNV-1a over the solutions' bytes) of icp_ldlt_solve6 on the systems of test_icp_solve.cpp (srand(7),
//                   B^T B + I) and on a generator of this file's own that also produces indefinite, rank-deficient and
//                   zero-diagonal matrices (every pivoting branch); tests/golden/icp_ldlt6_digests.txt holds the values of
//                   the header before the solve became a template on the size
//   three IN OUT    IN: m systems of 12 doubles (A row-major, b); OUT: m solutions of icp_ldlt_solve3, 3 doubles each
// -DM3D_TEST_ONLY_SIX leaves the second mode out (to print the digests from a header that has no 3 x 3 solve).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../misc3d_amd/csrc/m3d_icp_fp.hpp"

using namespace m3d;

static uint64_t fnv(uint64_t h, const double* x, int n) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(x);
    for (size_t k = 0; k < sizeof(double) * (size_t)n; ++k) h = (h ^ p[k]) * 1099511628211ull;
    return h;
}

static uint64_t lcg_state = 0x2545F4914F6CDD1Dull;
static double lcg() {   // in [-1, 1), 2^-20 steps: sums and products of a few of them are exact, ties of |diagonal| happen
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)((lcg_state >> 43) & 0x1FFFFF) / 1048576.0 - 1.0;
}

static int six() {
    double A[36], B[36], b[6], x[6];
    uint64_t h = 1469598103934665603ull;
    std::srand(7);
    auto rnd = [] { return (double)std::rand() / RAND_MAX * 2.0 - 1.0; };
    for (int trial = 0; trial < 2000; ++trial) {
        for (int k = 0; k < 36; ++k) B[k] = rnd();
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) {
                double v = (r == c) ? 1.0 : 0.0;
                for (int k = 0; k < 6; ++k) v += B[6 * k + r] * B[6 * k + c];
                A[6 * r + c] = v;
            }
        for (int k = 0; k < 6; ++k) b[k] = rnd();
        icp_ldlt_solve6(A, b, x);
        h = fnv(h, x, 6);
    }
    std::printf("%016llx\n", (unsigned long long)h);
    h = 1469598103934665603ull;
    for (int trial = 0; trial < 3000; ++trial) {
        const int kind = trial % 5;   // 0 symmetric indefinite, 1 rank k (< 6) B^T B, 2 a zero row and column, 3 diagonal with ties, 4 definite
        for (int k = 0; k < 36; ++k) A[k] = 0.0;
        if (kind == 0 || kind == 2) {
            for (int r = 0; r < 6; ++r)
                for (int c = r; c < 6; ++c) A[6 * r + c] = A[6 * c + r] = lcg();
            if (kind == 2) {
                const int z = trial % 6;
                for (int k = 0; k < 6; ++k) A[6 * z + k] = A[6 * k + z] = 0.0;
            }
        } else if (kind == 1 || kind == 4) {
            const int rank = kind == 1 ? 1 + trial % 5 : 6;
            for (int k = 0; k < 36; ++k) B[k] = lcg();
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c < 6; ++c) {
                    double v = kind == 4 && r == c ? 0.5 : 0.0;
                    for (int k = 0; k < rank; ++k) v += B[6 * k + r] * B[6 * k + c];
                    A[6 * r + c] = v;
                }
        } else {
            for (int r = 0; r < 6; ++r) A[7 * r] = (double)((trial / 5 + r) % 3) - 1.0;   // -1, 0, 1: equal |diagonal| entries
        }
        for (int k = 0; k < 6; ++k) b[k] = lcg();
        icp_ldlt_solve6(A, b, x);
        h = fnv(h, x, 6);
    }
    std::printf("%016llx\n", (unsigned long long)h);
    return 0;
}

#ifndef M3D_TEST_ONLY_SIX
static int three(const char* in, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    std::vector<double> sys;
    double rec[12];
    while (std::fread(rec, sizeof(double), 12, f) == 12) sys.insert(sys.end(), rec, rec + 12);
    std::fclose(f);
    std::FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    for (size_t t = 0; t < sys.size() / 12; ++t) {
        double x[3];
        icp_ldlt_solve3(sys.data() + 12 * t, sys.data() + 12 * t + 9, x);
        std::fwrite(x, sizeof(double), 3, o);
    }
    std::fclose(o);
    return 0;
}
#endif

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "six")) return six();
#ifndef M3D_TEST_ONLY_SIX
    if (argc == 4 && !std::strcmp(argv[1], "three")) return three(argv[2], argv[3]);
#endif
    return 64;
}
