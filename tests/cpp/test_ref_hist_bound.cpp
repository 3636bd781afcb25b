// Host-side check of the planes' reference-histogram bound (misc3d_amd/csrc/m3d_bound_fp.hpp: ref_plane_record, ref_bin,
// ref_hyp_record, ref_pair_ub -- the code ref_hist_tile and plane_bound_k run): no GPU, no library.  Random tiles of 512 points
// -- flat (a noisy or an exact plane patch), clutter, mixed -- in scenes scaled by 1e-2 .. 1e2 and moved up to 300 scene sizes from
// the origin; reference planes near the patch's plane and arbitrary ones, records in any scaling; hypotheses 0 .. 5 degrees off the
// reference, antiparallel to it, at the cosine limit on both sides, parallel and shifted by whole bins (the interval's ends land on
// bin edges) and by more than the histogram's span.  The histogram and the tile record are built the way ref_hist_tile builds them.
// For every (tile, hypothesis) pair the bound must be >= the exact count of the reference's test |((a x + b y) + c z) + d| < T.
// Built a second time with -DM3D_BOUND_NO_SLACK (no margins, inner bins only) it MUST report violations (tests/test_ref_hist_bound.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../misc3d_amd/csrc/m3d_bound_fp.hpp"

using namespace m3d;

static void cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
static void unit(double* v) {
    const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    v[0] /= n; v[1] /= n; v[2] /= n;
}

int main(int argc, char** argv) {
    const int trials = argc > 1 ? std::atoi(argv[1]) : 4000;
    std::mt19937_64 rng(20261019);
    std::uniform_real_distribution<double> U01(0.0, 1.0);
    std::normal_distribution<double> N01(0.0, 1.0);
    auto rdir = [&](double* v) { v[0] = N01(rng); v[1] = N01(rng); v[2] = N01(rng); unit(v); };
    long long pairs = 0, violations = 0, covered = 0, sum_ub = 0, sum_exact = 0;
    for (int t = 0; t < trials; ++t) {
        const double sc = std::pow(10.0, -2.0 + 4.0 * U01(rng));
        double off[3];
        rdir(off);
        const double far = sc * 300.0 * U01(rng) * (t % 4 == 0 ? 0.0 : 1.0);
        for (double& o : off) o *= far;
        const int kindt = t % 4;   // 0: flat, noisy   1: flat, exact   2: clutter   3: mixed
        const double ext = sc * (0.02 + 0.2 * U01(rng));
        const double sigma = kindt == 1 ? 0.0 : sc * std::pow(10.0, -4.0 + 2.0 * U01(rng));
        const double fplane = kindt == 2 ? 0.0 : (kindt == 3 ? 0.2 + 0.6 * U01(rng) : 1.0);
        double n0[3], a0[3], b0[3], tmp[3] = {1, 0, 0};
        rdir(n0);
        if (std::fabs(n0[0]) > 0.9) { tmp[0] = 0; tmp[1] = 1; }
        cross(n0, tmp, a0); unit(a0); cross(n0, a0, b0);
        const int npts = (t % 7 == 0) ? 100 + (int)(U01(rng) * 400) : 512;   // (a padded last tile: the rest is NaN)
        std::vector<double> P(512 * 3, NAN);
        double mabs = 0, lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int i = 0; i < npts; ++i) {
            double p[3];
            if (U01(rng) < fplane) {
                const double x = ext * (2 * U01(rng) - 1), y = ext * (2 * U01(rng) - 1), z = sigma * N01(rng);
                for (int k = 0; k < 3; ++k) p[k] = off[k] + x * a0[k] + y * b0[k] + z * n0[k];
            } else {
                for (int k = 0; k < 3; ++k) p[k] = off[k] + ext * (2 * U01(rng) - 1);
            }
            for (int k = 0; k < 3; ++k) {
                P[3 * i + k] = p[k];
                mabs = std::fmax(mabs, std::fabs(p[k]));
                lo[k] = std::fmin(lo[k], p[k]);
                hi[k] = std::fmax(hi[k], p[k]);
            }
        }
        mabs *= 1.0 + U01(rng);   // (the cloud's, not the tile's)
        const double base = sigma > 0 ? sigma : 1e-3 * sc;
        const double thr = base * std::pow(10.0, -0.5 + 1.5 * U01(rng));
        // ---- the reference plane: the patch's plane slightly off (what a lead pass finds), or any plane through the tile
        double ng[3], pg[3];
        if (t % 3 != 2) {
            double d[3]; rdir(d);
            for (int k = 0; k < 3; ++k) { ng[k] = n0[k] + 0.01 * U01(rng) * d[k]; pg[k] = off[k] + 2.0 * sigma * N01(rng) * n0[k]; }
        } else {
            rdir(ng);
            for (int k = 0; k < 3; ++k) pg[k] = off[k] + ext * (2 * U01(rng) - 1);
        }
        unit(ng);
        const double gs = std::pow(10.0, -1.0 + 2.0 * U01(rng));   // (records are not normalised)
        double grec[5];
        for (int k = 0; k < 3; ++k) grec[k] = ng[k] * gs;
        grec[3] = -((grec[0] * pg[0] + grec[1] * pg[1]) + grec[2] * pg[2]);
        grec[4] = thr * gs;
        const RefPlane g = ref_plane_record(grec, mabs);
        // ---- ref_hist_tile on the host
        std::vector<uint16_t> cum(kRefCumStride, 0);
        std::vector<int> hist(kRefBins + 2, 0);
        double c[3], r2 = 0;
        for (int k = 0; k < 3; ++k) c[k] = 0.5 * lo[k] + 0.5 * hi[k];
        for (int i = 0; i < 512; ++i) {
            if (!(P[3 * i] == P[3 * i])) continue;
            const double dx = P[3 * i] - c[0], dy = P[3 * i + 1] - c[1], dz = P[3 * i + 2] - c[2];
            r2 = std::fmax(r2, (dx * dx + dy * dy) + dz * dz);
            const double s = ((g.a * P[3 * i] + g.b * P[3 * i + 1]) + g.c * P[3 * i + 2]) + g.d;
            hist[ref_bin(s, g.invw)]++;
        }
        for (int k = 0; k < kRefBins + 2; ++k) cum[k + 1] = (uint16_t)(cum[k] + hist[k]);
        const double trec[kRefTileStride] = {c[0], c[1], c[2], ((g.a * c[0] + g.b * c[1]) + g.c * c[2]) + g.d,
                                             std::sqrt(r2) * (1.0 + 1e-12)};
        // ---- hypotheses
        for (int hq = 0; hq < 48; ++hq) {
            double rec[5];
            const int how = hq % 6;
            const double hs = std::pow(10.0, -1.0 + 2.0 * U01(rng));
            double T = thr * std::pow(10.0, -0.3 + 0.8 * U01(rng));
            if (how <= 2 || how == 5) {
                // 0: 0 .. 5 degrees off g   1: the same, antiparallel   2: at the cosine limit, just inside or just outside
                // 5: 0 .. 0.5 degrees (the hypotheses that matter in a fit)
                double ax[3], q[3];
                rdir(q); cross(ng, q, ax); unit(ax);   // a direction orthogonal to ng
                const double lim = std::acos(kRefMinCos);
                const double th = how == 2 ? lim * (1.0 + (U01(rng) < 0.5 ? -1.0 : 1.0) * std::pow(10.0, -12.0 + 11.0 * U01(rng)))
                                           : (how == 5 ? 0.5 : 5.0) * U01(rng) * M_PI / 180.0;
                double n[3], p0[3];
                for (int k = 0; k < 3; ++k) n[k] = std::cos(th) * ng[k] + std::sin(th) * ax[k];
                const double sh = 3.0 * thr * N01(rng);
                for (int k = 0; k < 3; ++k) p0[k] = pg[k] + sh * ng[k] + (how == 5 ? 0.0 : ext * (2 * U01(rng) - 1)) * ax[k];
                const double sgn = how == 1 ? -1.0 : 1.0;
                for (int k = 0; k < 3; ++k) rec[k] = sgn * hs * n[k];
                rec[3] = -((rec[0] * p0[0] + rec[1] * p0[1]) + rec[2] * p0[2]);
            } else {
                // 3: parallel to g, shifted by a whole number of bins, T a whole number of bins: the ends land on bin edges
                // 4: parallel, shifted beyond the histogram's span (the tails)
                const double w = thr * 8.0 / kRefBins;   // a bin, in units of distance
                const double sh = how == 3 ? w * (double)((int)(U01(rng) * 2 * kRefBins) - kRefBins) : thr * (3.0 + 9.0 * U01(rng)) * (U01(rng) < 0.5 ? -1.0 : 1.0);
                if (how == 3) T = w * (double)(1 + (int)(U01(rng) * kRefBins / 4));
                const double sgn = (hq & 8) ? -1.0 : 1.0;
                const double f = (hq & 16) ? hs / gs : 1.0;   // (the same plane in another scaling, or g's own)
                for (int k = 0; k < 3; ++k) rec[k] = sgn * f * grec[k];
                rec[3] = sgn * f * (grec[3] + gs * sh);
                rec[4] = T * f * gs;   // (T in the record's scaling)
            }
            if (how <= 2 || how == 5) rec[4] = T * hs;
            int exact = 0;
            for (int i = 0; i < 512; ++i) {
                const double s64 = ((rec[0] * P[3 * i] + rec[1] * P[3 * i + 1]) + rec[2] * P[3 * i + 2]) + rec[3];
                exact += std::fabs(s64) < rec[4];
            }
            const RefHypRec rr = ref_hyp_record(g, rec, mabs);
            const uint32_t ub = ref_pair_ub(rr, rec[0], rec[1], rec[2], rec[3], trec, cum.data());
            ++pairs;
            if (rr.ok) { ++covered; sum_ub += ub; sum_exact += exact; }
            if ((long long)ub < exact) {
                if (violations < 5) std::printf("VIOLATION trial %d hyp %d: ub %u < exact %d (kind %d, how %d, sc %.3g, far %.3g, sigma %.3g, T %.3g)\n", t, hq, ub, exact, kindt, how, sc, far, sigma, T);
                ++violations;
            }
        }
    }
    std::printf("%d bins: %lld pairs covered by the reference bound, sum of bounds %lld, sum of exact counts %lld\n", kRefBins, covered, sum_ub, sum_exact);
    std::printf("%lld (tile, hypothesis) pairs, violations %lld\n", pairs, violations);
    if (violations == 0 && covered * 10 > pairs * 8) std::printf("all checks passed\n");
    return (violations == 0 && covered * 10 > pairs * 8) ? 0 : 1;
}
