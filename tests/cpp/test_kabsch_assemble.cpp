// test_kabsch_assemble.cpp -- host-side run of the pose assembly m3d_kabsch applies to its 18 device sums
// (misc3d_amd/csrc/m3d_reg_fp.hpp umeyama_from_sums: the text the library compiles): no GPU, no library.  Reads per line
//   <n> <scaling 0|1> h[18]
// every double as the 16 hex digits of its bit pattern, and prints the 16 entries of T as hex words.
// tests/test_gpu_reg_sums.py feeds it what m3d_bench_kabsch_sums returned and holds m3d_kabsch's pose to the output bit for bit.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../misc3d_amd/csrc/m3d_reg_fp.hpp"

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? std::fopen(argv[1], "r") : stdin;
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    unsigned long long n;
    int scaling, lines = 0;
    while (std::fscanf(f, "%llu %d", &n, &scaling) == 2) {
        double h[18], T[16];
        for (int k = 0; k < 18; ++k) {
            uint64_t w;
            if (std::fscanf(f, "%" SCNx64, &w) != 1) return 2;
            std::memcpy(&h[k], &w, 8);
        }
        m3d::umeyama_from_sums(h, (double)n, scaling != 0, T);
        for (int k = 0; k < 16; ++k) {
            uint64_t w;
            std::memcpy(&w, &T[k], 8);
            std::printf("%s%016" PRIx64, k ? " " : "", w);
        }
        std::printf("\n");
        ++lines;
    }
    if (f != stdin) std::fclose(f);
    return lines ? 0 : 2;
}
