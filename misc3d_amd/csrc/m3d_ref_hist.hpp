// m3d_ref_hist.hpp -- the reference-plane histograms of a plane fit (device only; arithmetic: m3d_bound_fp.hpp, ref_*).
//
// A tile's stored histogram (tile_frames_k) runs along the tile's own thin direction; a clutter tile has none, and plane_pair_ub
// prices it at up to all of its points for a hypothesis that has twenty inliers there.  But every hypothesis that matters in a fit
// lies within a fraction of a degree of ONE plane, and that plane is known before the bound runs: g, the best hypothesis of the
// fit's lead pass.  ref_hist_tile -- one wave per tile, once per fit -- bins the tile's points by their signed distance to g
// (fp64, the scoring expression) over kRefBins bins of T_g 8 / kRefBins centred on 0, with two tails, and stores the cumulative
// counts with the tile's box centre c, S_g(c) and rho >= |p - c|: ref_pair_ub then bounds every near-parallel hypothesis tightly on
// every tile, clutter included (plane_bound_k takes the smaller of the two bounds).
//
// g: the valid leading hypothesis with the highest count, the lowest index among equals, folded from the lead's counter replicas by
// EVERY wave for itself (the same loads, the same maximum: the same g) -- or `fixed_index` (counts_rep null: the bench hook).
// No such hypothesis, one with fewer than min_count inliers, or a record ref_plane_record refuses: hdr[0] = 0, the tiles are not
// read and plane_bound_k runs as it did.
#pragma once
#include "m3d_bound_fp.hpp"
#include "m3d_cull_kernels.hpp"
#include "m3d_wave.hpp"

namespace m3d {

constexpr int kRefHistPerLane = (kRefBins + 3 + 63) / 64;   // histogram slots per lane of the cumulative scan
constexpr int kRefHistWords = 64 * kRefHistPerLane;         // LDS words ref_hist_tile needs

__device__ __forceinline__ void ref_hist_tile(const RefHistArgs& a, uint32_t tile, uint32_t* hist /* LDS: kRefHistWords */) {
    const int lane = threadIdx.x & 63;
    uint32_t hg = a.fixed_index;
    bool have = true;
    if (a.counts_rep) {
        unsigned long long key = 0;   // (count << 32 | ~index): lead_fold_keep_k's pick
        for (uint32_t h = lane; h < a.lead; h += 64u) {
            uint32_t c = 0;
#pragma unroll
            for (int r = 0; r < kCountReplicas; ++r) c += a.counts_rep[(size_t)r * a.rep_stride + h];
            const bool ok = h < a.h_count && a.valid[h];
            if (ok && c) key = max(key, ((unsigned long long)c << 32) | (0xFFFFFFFFu - h));
        }
        key = wave_max(key);
        // the gate: a lead whose best plane holds fewer than min_count points has found no structure (uniform clutter) -- the
        // survivor list will be too long for plane_bound_k to bound anything, and the tiles' 24 bytes per point stay unread
        have = key != 0ull && (uint32_t)(key >> 32) >= a.min_count;
        hg = 0xFFFFFFFFu - (uint32_t)key;
    }
    hg = (uint32_t)__builtin_amdgcn_readfirstlane((int)hg);
    RefPlane g;
    g.ok = false;
    if (have) g = ref_plane_record(a.score + (size_t)hg * kModelStride, a.max_abs);   // (wave-uniform)
    have = have && g.ok;
    if (tile == 0 && lane == 0) {
        a.hdr[0] = have ? 1.0 : 0.0;
        if (have)
            for (int k = 0; k < 5; ++k) a.hdr[1 + k] = a.score[(size_t)hg * kModelStride + k];
        a.hdr[6] = (double)hg;
    }
    if (!have) return;   // (wave-uniform)
    // (measured: these loads in front of the fold, in flight under it, 12.0 instead of 13.3 us for the launch on a cloud with a
    //  plane -- and 8 us more per fit on uniform clutter, where they are for nothing: profiles/r09_ref_bound.txt)
    constexpr int P = kTilePoints / 64;
    double px[P], py[P], pz[P];
    bool fin[P];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t nf = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const size_t i = (size_t)tile * kTilePoints + j * 64 + lane;
        px[j] = a.sx[i];
        py[j] = a.sy[i];
        pz[j] = a.sz[i];
        fin[j] = (px[j] * 0.0 == 0.0) && (py[j] * 0.0 == 0.0) && (pz[j] * 0.0 == 0.0);
        if (fin[j]) {
            lo[0] = fmin(lo[0], px[j]); hi[0] = fmax(hi[0], px[j]);
            lo[1] = fmin(lo[1], py[j]); hi[1] = fmax(hi[1], py[j]);
            lo[2] = fmin(lo[2], pz[j]); hi[2] = fmax(hi[2], pz[j]);
            ++nf;
        }
    }
    for (int k = 0; k < 3; ++k) {
        lo[k] = wave_min(lo[k]);
        hi[k] = wave_max(hi[k]);
    }
    nf = wave_sum(nf);
    double c[3] = {0.0, 0.0, 0.0};
    if (nf)
        for (int k = 0; k < 3; ++k) c[k] = 0.5 * lo[k] + 0.5 * hi[k];
    for (int i = lane; i < kRefHistWords; i += 64) hist[i] = 0u;
    __syncthreads();
    double r2 = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        if (!fin[j]) continue;   // (NaN padding, tombstones, infinities: inliers of no plane)
        const double dx = px[j] - c[0], dy = py[j] - c[1], dz = pz[j] - c[2];
        r2 = fmax(r2, (dx * dx + dy * dy) + dz * dz);
        const double s = ((g.a * px[j] + g.b * py[j]) + g.c * pz[j]) + g.d;
        atomicAdd(&hist[ref_bin(s, g.invw)], 1u);
    }
    r2 = wave_max(r2);
    __syncthreads();
    {   // cum[k] = points with bin < k, k = 0 .. kRefBins + 2
        uint32_t own = 0;
#pragma unroll
        for (int i = 0; i < kRefHistPerLane; ++i) own += hist[lane * kRefHistPerLane + i];   // (slots past the last bin are zero)
        uint32_t run = wave_incl_scan(own, lane) - own;
        uint16_t* __restrict__ cm = a.cum + (size_t)tile * kRefCumStride;
#pragma unroll
        for (int i = 0; i < kRefHistPerLane; ++i) {
            const int idx = lane * kRefHistPerLane + i;
            if (idx <= kRefBins + 2) cm[idx] = (uint16_t)run;
            run += hist[idx];
        }
    }
    if (lane == 0) {
        double* __restrict__ t = a.tiles + (size_t)tile * kRefTileStride;
        t[0] = c[0]; t[1] = c[1]; t[2] = c[2];
        t[3] = ((g.a * c[0] + g.b * c[1]) + g.c * c[2]) + g.d;
        t[4] = sqrt(r2) * (1.0 + 1e-12);
    }
}

}  // namespace m3d
