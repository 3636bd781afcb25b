// test_ppf_mirror.cpp -- the host build of misc3d_amd/csrc/m3d_ppf_fp.hpp (the text the PPF kernels compile) against
// hand-computed bins, edge values included.  No GPU, no library: g++ -O2 -std=c++17 -ffp-contract=off.  Prints "ok" and
// returns 0, or the first failures and 1.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../misc3d_amd/csrc/m3d_ppf_fp.hpp"

using namespace m3d;

static int g_fail = 0;
#define CHECK_EQ(got, want)                                                                          \
    do {                                                                                             \
        const long long g_ = (long long)(got), w_ = (long long)(want);                               \
        if (g_ != w_ && ++g_fail < 20) std::printf("line %d: %s = %lld, want %lld\n", __LINE__, #got, g_, w_); \
    } while (0)

int main() {
    const double step = M_PI / 15.0;   // 12 degrees
    const PpfSizes s = ppf_sizes(1.0, 0.05, step);
    CHECK_EQ(s.angle_num, 16);
    CHECK_EQ(s.alpha_num, 31);
    CHECK_EQ(s.dist_num, 21);
    CHECK_EQ(s.table_size, 16 * 16 * 16 * 21);
    PpfTables T, T3;
    std::vector<double> e2, e2b;
    ppf_make_tables(s, step, true, &T, &e2);
    ppf_make_tables(s, step, false, &T3, &e2b);
    CHECK_EQ(T.spread_k, 2);
    CHECK_EQ(T3.spread_k, 3);
    // other steps: 11.25 degrees -> 33 bins, 6 -> 61, 5.625 -> 65 (refused by the library: > 64)
    CHECK_EQ(ppf_sizes(1.0, 0.05, M_PI / 16.0).alpha_num, 33);
    CHECK_EQ(ppf_sizes(1.0, 0.05, M_PI / 30.0).alpha_num, 61);
    CHECK_EQ(ppf_sizes(1.0, 0.05, M_PI / 32.0).alpha_num, 65);

    // round(acos(x) / step)
    CHECK_EQ(ppf_angle_bin(T, 1.0), 0);
    CHECK_EQ(ppf_angle_bin(T, 1.0000001), 0);          // acos is NaN in the reference: the end bin
    CHECK_EQ(ppf_angle_bin(T, -1.0), 15);
    CHECK_EQ(ppf_angle_bin(T, -1.0000001), 15);
    CHECK_EQ(ppf_angle_bin(T, std::cos(5.9 * M_PI / 180.0)), 0);
    CHECK_EQ(ppf_angle_bin(T, std::cos(6.1 * M_PI / 180.0)), 1);
    CHECK_EQ(ppf_angle_bin(T, 0.6), 4);                // 53.13 degrees
    CHECK_EQ(ppf_angle_bin(T, 0.36), 6);               // 68.90 degrees
    CHECK_EQ(ppf_angle_bin(T, -0.5), 10);              // 120 degrees
    for (int k = 0; k < 15; ++k) {                     // an edge belongs to the upper bin (round half away from zero)
        CHECK_EQ(ppf_angle_bin(T, T.cos_edge[k]), k + 1);
        CHECK_EQ(ppf_angle_bin(T, std::nextafter(T.cos_edge[k], 2.0)), k);
    }

    // round(sqrt(d2) / dist_step), dist_step = 0.05
    CHECK_EQ(ppf_dist_bin(T, 0.5 * 0.5), 10);
    CHECK_EQ(ppf_dist_bin(T, 1e-12), 0);
    CHECK_EQ(ppf_dist_bin(T, 1.0), 20);
    CHECK_EQ(ppf_dist_bin(T, 1.03 * 1.03), 21);        // beyond the table: the pair is skipped
    CHECK_EQ(ppf_dist_bin(T, INFINITY), 21);
    for (int k = 0; k < 21; ++k) {
        CHECK_EQ(ppf_dist_bin(T, T.dist_edge2[k]), k + 1);
        CHECK_EQ(ppf_dist_bin(T, std::nextafter(T.dist_edge2[k], 0.0)), k);
    }

    // round((atan2(-z, y) + pi) / step)
    CHECK_EQ(ppf_alpha_bin(T, 1.0, 0.0), 15);          // alpha = -0
    CHECK_EQ(ppf_alpha_bin(T, 1.0, -0.0), 15);         // alpha = +0
    CHECK_EQ(ppf_alpha_bin(T, -1.0, 0.0), 0);          // atan2(-0, -1) = -pi
    CHECK_EQ(ppf_alpha_bin(T, -1.0, -0.0), 30);        // atan2(+0, -1) = +pi
    CHECK_EQ(ppf_alpha_bin(T, 0.0, 0.0), 15);          // counts as alpha = 0
    for (int b = 0; b < 30; ++b) {
        const double lo = -M_PI + (b + 0.3) * step, hi = -M_PI + (b + 0.7) * step;
        CHECK_EQ(ppf_alpha_bin(T, 2.5 * std::cos(lo), -2.5 * std::sin(lo)), b);
        CHECK_EQ(ppf_alpha_bin(T, 0.01 * std::cos(hi), -0.01 * std::sin(hi)), b + 1);
        // on the edge direction itself the cross product is c s - s c = 0: the upper bin; a nanoradian before it: the lower
        CHECK_EQ(ppf_alpha_bin(T, T.alpha_c[b], -T.alpha_s[b]), b + 1);
        const double th = -M_PI + (b + 0.5) * step - 1e-9;
        CHECK_EQ(ppf_alpha_bin(T, std::cos(th), -std::sin(th)), b);
    }

    // a pair by hand: p0 at the origin with normal +x (its frame is the identity), p1 = (0.3, 0.4, 0), n1 = (0.6, 0, 0.8)
    const double p0[3] = {0, 0, 0}, n0[3] = {1, 0, 0}, p1[3] = {0.3, 0.4, 0.0}, n1[3] = {0.6, 0.0, 0.8};
    const double frame[8] = {0, 1, 0, 0, 0, 0, 1, 0};
    int q[4], qa = -1;
    CHECK_EQ(ppf_pair_bins(T, p0, n0, p1, n1, frame, q, &qa), 1);
    CHECK_EQ(q[0], 4);    // acos(0.6)
    CHECK_EQ(q[1], 6);    // acos(0.36)
    CHECK_EQ(q[2], 4);    // acos(0.6)
    CHECK_EQ(q[3], 10);   // 0.5 / 0.05
    CHECK_EQ(qa, 15);     // atan2(-0, 0.4)
    CHECK_EQ(ppf_cell(T, q), 4 + 16 * (6 + 16 * (4 + 16 * 10)));
    CHECK_EQ(ppf_pair_bins(T, p0, n0, p0, n1, frame, q, &qa), 0);                 // d2 == 0
    const double far[3] = {0.9, 0.9, 0.9};
    CHECK_EQ(ppf_pair_bins(T, p0, n0, far, n1, frame, q, &qa), 0);                // 1.56 / 0.05 > 20.5
    CHECK_EQ(ppf_alpha_index(3, 29, 31), 5);
    CHECK_EQ(ppf_alpha_index(29, 3, 31), 26);

    // SpreadPPF: 24 / 81 cells in the interior, fewer at the ends
    auto count = [](const PpfTables& t, int a0, int a1, int a2, int d) {
        const int qq[4] = {a0, a1, a2, d};
        int c = 0;
        for (int k = 0; k < ppf_spread_count(t); ++k) c += ppf_spread_cell(t, qq, k) >= 0 ? 1 : 0;
        return c;
    };
    CHECK_EQ(ppf_spread_count(T), 24);
    CHECK_EQ(ppf_spread_count(T3), 81);
    CHECK_EQ(count(T, 5, 5, 5, 5), 24);
    CHECK_EQ(count(T3, 5, 5, 5, 5), 81);
    CHECK_EQ(count(T, 0, 0, 0, 0), 2);        // the distance keeps {0, +1}, each angle of {-1, 0} only 0
    CHECK_EQ(count(T3, 0, 0, 0, 0), 16);
    CHECK_EQ(count(T, 15, 15, 15, 20), 16);   // {-1, 0} on everything
    CHECK_EQ(count(T3, 15, 15, 15, 20), 16);
    CHECK_EQ(count(T, 0, 5, 15, 10), 12);     // 3 x 1 x 2 x 2
    {
        const int qq[4] = {5, 6, 7, 8};       // the loop nest's order: s0 (distance) outermost, s3 (third angle) innermost
        CHECK_EQ(ppf_spread_cell(T, qq, 0), 4 + 16 * (5 + 16 * (6 + 16 * 7)));
        CHECK_EQ(ppf_spread_cell(T, qq, 1), 4 + 16 * (5 + 16 * (7 + 16 * 7)));
        CHECK_EQ(ppf_spread_cell(T, qq, 23), 5 + 16 * (6 + 16 * (7 + 16 * 9)));
    }
    // the pair filter: closer than the distance threshold AND normals within the angle threshold
    const double na[3] = {0, 0, 1}, nb[3] = {0, 0.6, 0.8};
    CHECK_EQ(ppf_pair_filtered(0.01, na, na, 0.2, std::cos(M_PI / 6)), 1);
    CHECK_EQ(ppf_pair_filtered(0.01, na, nb, 0.2, std::cos(M_PI / 6)), 0);   // 36.9 degrees apart
    CHECK_EQ(ppf_pair_filtered(0.09, na, na, 0.2, std::cos(M_PI / 6)), 0);   // 0.3 away
    if (g_fail) {
        std::printf("%d failures\n", g_fail);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
