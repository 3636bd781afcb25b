// test_generalfit_fp.cpp -- host-side run of GeneralFit's closed forms (misc3d_amd/csrc/m3d_generalfit_fp.hpp: the text the
// library compiles): no GPU, no library.  Reads moment sets that tests/test_generalfit.py has computed exactly and rounded
// once, one per line, every double as the 16 hex digits of its bit pattern:
//   <kind 0|1> 0 <n> c0[3] raw[12]        raw moments about c0     -> moments_about_mean -> the closed form
//   <kind 0|1> 1 <n> mean[3] centred[10]  the centred moments      -> the closed form
// and prints per line "<ok 0|1> p0 p1 p2 p3" as hex words.  The test holds them to the exact reference: an error here is the
// closed form's, not the sums'.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../misc3d_amd/csrc/m3d_generalfit_fp.hpp"

static bool read_double(FILE* f, double* v) {
    uint64_t w;
    if (std::fscanf(f, "%" SCNx64, &w) != 1) return false;
    std::memcpy(v, &w, 8);
    return true;
}

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? std::fopen(argv[1], "r") : stdin;
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    int kind, mode;
    unsigned long long n;
    int lines = 0;
    while (std::fscanf(f, "%d %d %llu", &kind, &mode, &n) == 3) {
        if (kind < 0 || kind > 1 || mode < 0 || mode > 1 || n == 0) {
            std::fprintf(stderr, "line %d: bad header\n", lines + 1);
            return 2;
        }
        double head[3], mean[3], centred[10];
        for (int k = 0; k < 3; ++k)
            if (!read_double(f, &head[k])) return 2;
        if (mode == 0) {
            double raw[12];
            for (int k = 0; k < 12; ++k)
                if (!read_double(f, &raw[k])) return 2;
            m3d::moments_about_mean(raw, head, (double)n, mean, centred);
        } else {
            for (int k = 0; k < 3; ++k) mean[k] = head[k];
            for (int k = 0; k < 10; ++k)
                if (!read_double(f, &centred[k])) return 2;
        }
        double out[4] = {0.0, 0.0, 0.0, 0.0};
        const bool ok = kind == 0 ? m3d::plane_from_moments(mean, centred, out) : m3d::sphere_from_moments(mean, centred, (double)n, out);
        std::printf("%d", ok ? 1 : 0);
        for (int k = 0; k < 4; ++k) {
            uint64_t w;
            std::memcpy(&w, &out[k], 8);
            std::printf(" %016" PRIx64, w);
        }
        std::printf("\n");
        ++lines;
    }
    if (f != stdin) std::fclose(f);
    return lines ? 0 : 2;
}
