// m3d_kernels.hip -- hand-written gfx950 (MI355X / CDNA4) kernels of the Misc3D RANSAC hot path.
//
// Replaces these reference loops (paths relative to the Misc3D repository):
//   minimal_fit_k   include/misc3d/common/ransac.h:576-582 (SelectByIndex + MinimalFit per hypothesis)
//   score_*_k       ransac.h:626-641 (EvaluateModel's scan over N points) x ransac.h:572 (H hypotheses)
//   compact_*_k     ransac.h:537-543 (RefineModel's inlier list), src/iterative_plane_segmentation.cpp:32-33
//   sum_*_k         ransac.h:164-188 (GeneralFit sums)
//
// Design notes (DESIGN.md has the long form):
//   * Scoring is a count-only kernel.  Each lane keeps kScoreP points in VGPRs for the whole launch,
//     hypothesis records are wave-uniform and come in through scalar loads, the `d < thr` test is
//     replaced by an EXACT per-hypothesis cut-off on the pre-sqrt / pre-divide quantity
//     (m3d_fp.hpp), so the inner loop is 6 (plane) / 8 (sphere) / 20 (cylinder) fp64 VALU ops plus
//     the compare, with v_cmp -> s_bcnt1 -> s_add counting on the scalar unit.
//   * No FMA contraction anywhere: products and sums round separately like the reference's x86-64
//     SSE2 build.  The file is compiled with -ffp-contract=off and carries the pragma as well.
//   * Integer results only (counts, indices) leave the scoring path; fp64 sums that the reference
//     forms serially are either reproduced serially (serial_sum_k) or are tolerance-checked
//     parameters (GeneralFit), never inlier decisions.
#include <cstdio>
#include <cstdlib>
#include "m3d_kernels.hpp"
#include "m3d_config.hpp"
#include "m3d_poison.hpp"

#include "m3d_fp.hpp"
#include "m3d_wave.hpp"

#pragma clang fp contract(off)

namespace m3d {

// ------------------------------------------------------------------------------------------------
// K0  AoS -> SoA
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void aos_to_soa_k(const double* __restrict__ aos,
                                                     double* __restrict__ x, double* __restrict__ y,
                                                     double* __restrict__ z, uint32_t n,
                                                     uint32_t n_pad) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_pad) return;
    const double nan = u2f(0x7FF8000000000000ull);
    double px = nan, py = nan, pz = nan;
    if (i < n) {
        px = aos[3 * (size_t)i];
        py = aos[3 * (size_t)i + 1];
        pz = aos[3 * (size_t)i + 2];
    }
    x[i] = px;
    y[i] = py;
    z[i] = pz;
}

void launch_aos_to_soa(const double* aos, double* x, double* y, double* z, uint32_t n,
                       uint32_t n_pad, hipStream_t s) {
    if (n_pad == 0) return;
    aos_to_soa_k<<<(n_pad + 255) / 256, 256, 0, s>>>(aos, x, y, z, n, n_pad);
}

// Bounding box of the finite points + their number (the Hilbert sort's grid): per-workgroup partials, then one
// workgroup folds them.  out[0..2] = lo, out[3..5] = hi, out[6] = count (exact in a double: n < 2^31).
constexpr int kBboxBlocks = 1024;
__device__ __forceinline__ void bbox_fold(double (&v)[7], double (*red)[7]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        double a = v[k];
        for (int off = 32; off > 0; off >>= 1) {
            const double b = __shfl_xor(a, off, 64);
            a = k < 3 ? fmin(a, b) : (k < 6 ? fmax(a, b) : a + b);
        }
        if (lane == 0) red[wave][k] = a;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const double a = red[0][k], b = red[1][k], c = red[2][k], d = red[3][k];
        v[k] = k < 3 ? fmin(fmin(a, b), fmin(c, d)) : (k < 6 ? fmax(fmax(a, b), fmax(c, d)) : (a + b) + (c + d));
    }
}
__global__ __launch_bounds__(256) void bbox_partial_k(const double* __restrict__ x, const double* __restrict__ y,
                                                       const double* __restrict__ z, uint32_t n,
                                                       double* __restrict__ partial) {
    __shared__ double red[4][7];
    const double inf = u2f(0x7FF0000000000000ull);
    double v[7] = {inf, inf, inf, -inf, -inf, -inf, 0.0};
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const double px = x[i], py = y[i], pz = z[i];
        if (isfinite(px) && isfinite(py) && isfinite(pz)) {
            v[0] = fmin(v[0], px); v[1] = fmin(v[1], py); v[2] = fmin(v[2], pz);
            v[3] = fmax(v[3], px); v[4] = fmax(v[4], py); v[5] = fmax(v[5], pz);
            v[6] += 1.0;
        }
    }
    bbox_fold(v, red);
    if (threadIdx.x < 7) partial[blockIdx.x * 8 + threadIdx.x] = v[threadIdx.x];
}
__global__ __launch_bounds__(256) void bbox_final_k(const double* __restrict__ partial, uint32_t blocks,
                                                     double* __restrict__ out) {
    __shared__ double red[4][7];
    const double inf = u2f(0x7FF0000000000000ull);
    double v[7] = {inf, inf, inf, -inf, -inf, -inf, 0.0};
    for (uint32_t b = threadIdx.x; b < blocks; b += 256u) {
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const double t = partial[b * 8 + k];
            v[k] = k < 3 ? fmin(v[k], t) : (k < 6 ? fmax(v[k], t) : v[k] + t);
        }
    }
    bbox_fold(v, red);
    if (threadIdx.x < 7) out[threadIdx.x] = v[threadIdx.x];
}
void launch_bbox(const double* x, const double* y, const double* z, uint32_t n, double* partial, double* out,
                 hipStream_t s) {
    const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(kBboxBlocks, (n + 255) / 256));
    bbox_partial_k<<<blocks, 256, 0, s>>>(x, y, z, n, partial);
    bbox_final_k<<<1, 256, 0, s>>>(partial, blocks, out);
}

__global__ void iota_k(uint32_t* v, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) v[i] = i;
}
void launch_iota(uint32_t* v, uint32_t n, hipStream_t s) {
    if (n) iota_k<<<(n + 255) / 256, 256, 0, s>>>(v, n);
}

// ------------------------------------------------------------------------------------------------
// K1  minimal fit + exact cut-offs, one thread per hypothesis
// ------------------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(64) void minimal_fit_k(CloudView c, const uint32_t* __restrict__ samples,
                                                     uint32_t h_count, uint32_t h_pad, double thr,
                                                     double* __restrict__ score,
                                                     double* __restrict__ params,
                                                     uint8_t* __restrict__ valid, uint32_t* __restrict__ zero_u32, uint32_t* __restrict__ zero_u32b,
                                                     uint32_t* __restrict__ zero_one, LeadPrep lead, double cull_max_abs,
                                                     Cull32Out c32, PoisonJob poison, uint32_t fit_blocks) {
    // workgroups behind the fit's own: the previous segmentation round's tombstone pass, one wave per tile of the sorted
    // copy (m3d_poison.hpp) -- two latency-bound launches in the time of the longer one
    if (KIND == 0 && blockIdx.x >= fit_blocks) {   // (workgroup-uniform)
        poison_tile(poison, blockIdx.x - fit_blocks, (int)threadIdx.x);
        return;
    }
    const uint32_t h = blockIdx.x * 64u + threadIdx.x;
    if (h >= h_pad) return;
    if (zero_u32 && h + 1 < h_pad) zero_u32[h] = 0;   // per-hypothesis counter cleared on the way (saves a memset launch)
    if (zero_u32b && h + 1 < h_pad) zero_u32b[h] = 0;   // (the phase counters of the box tests: launch_score_phased)
    if (zero_one && h < 8) zero_one[h] = 0;           // a fit's first chunk: the running best count + the pick's ticket, key and key2 (PickFinal), the survivor list's length (plane_bound_k)
    if (lead.counts_rep) {
        // a fit's first chunk: what keep_mask_k would do for the leading hypotheses (nothing to prune against yet: keep
        // everything; clear their counter replicas and the launch's pair counters) -- one launch less in front of the lead pass
        if (h < lead.n_lead) {
            for (uint32_t r = 0; r < lead.n_rep; ++r) lead.counts_rep[(size_t)r * lead.rep_stride + h] = 0u;
            if ((h & 63u) == 0u) lead.keep[h >> 6] = ~0ull;
        }
        if (h < lead.n_pair) lead.counts_rep[(size_t)lead.n_rep * lead.rep_stride + h] = 0u;
    }
    const double nan = u2f(0x7FF8000000000000ull);
    double rec[kModelStride];
    double par[kModelStride];
    for (int k = 0; k < kModelStride; ++k) {
        rec[k] = 0.0;
        par[k] = 0.0;
    }
    bool ok = false;
    if (h < h_count) {
        if (KIND == 0) {
            double p[9];
            for (int s = 0; s < 3; ++s) {
                const uint32_t i = samples[3 * (size_t)h + s];
                p[3 * s] = c.x[i];
                p[3 * s + 1] = c.y[i];
                p[3 * s + 2] = c.z[i];
            }
            ok = plane_minimal_fit(p, p + 3, p + 6, par);
            if (ok) {
                // spare slots of the PARAMETER record: the first sample point, an inlier of the model -- the provisional
                // centre RefineModel's fused moment sums are taken about (compact_count_k<.., true>)
                par[4] = p[0];
                par[5] = p[1];
                par[6] = p[2];
                rec[0] = par[0];
                rec[1] = par[1];
                rec[2] = par[2];
                rec[3] = par[3];
                rec[4] = plane_cutoff(par, thr);
                // cut-off of the BOX tests (cull_tiles_k), the rounding margin taken once per hypothesis: every |a x|,
                // |b y|, |c z| of the cloud is at most |.| * max_abs, so mag <= (|a| + |b| + |c|) max_abs + |d| for every
                // box AND every point; a box is culled when |s| - r > T + 1e-12 (mag + T)
                {
                    const double mag = ((fabs(par[0]) + fabs(par[1])) + fabs(par[2])) * cull_max_abs + fabs(par[3]);
                    rec[5] = rec[4] + 1e-12 * (mag + rec[4]);
                }
            }
        } else if (KIND == 1) {
            double p[12];
            for (int s = 0; s < 4; ++s) {
                const uint32_t i = samples[4 * (size_t)h + s];
                p[3 * s] = c.x[i];
                p[3 * s + 1] = c.y[i];
                p[3 * s + 2] = c.z[i];
            }
            ok = sphere_minimal_fit(p, par);
            if (ok) {
                // spare slots of the PARAMETER record, as for the plane: the provisional centre of RefineModel's fused moment
                // sums -- the centroid of the four sample points, which lies among the inliers (each sample point is one) and
                // IS their mean when they are the only inliers; not the model's centre (see compact_count_k)
                par[4] = ((p[0] + p[3]) + (p[6] + p[9])) * 0.25;
                par[5] = ((p[1] + p[4]) + (p[7] + p[10])) * 0.25;
                par[6] = ((p[2] + p[5]) + (p[8] + p[11])) * 0.25;
                rec[0] = par[0];
                rec[1] = par[1];
                rec[2] = par[2];
                sphere_cutoffs(par, thr, &rec[3], &rec[4]);
            }
        } else {
            double p[6], nn[6];
            for (int s = 0; s < 2; ++s) {
                const uint32_t i = samples[2 * (size_t)h + s];
                p[3 * s] = c.x[i];
                p[3 * s + 1] = c.y[i];
                p[3 * s + 2] = c.z[i];
                nn[3 * s] = c.nx[i];
                nn[3 * s + 1] = c.ny[i];
                nn[3 * s + 2] = c.nz[i];
            }
            ok = cylinder_minimal_fit(p, nn, par);
            if (ok) {
                double ref[3], L;
                cylinder_ref(par, ref, &L);
                rec[0] = par[0];
                rec[1] = par[1];
                rec[2] = par[2];
                rec[3] = ref[0];
                rec[4] = ref[1];
                rec[5] = ref[2];
                cylinder_cutoffs(par, thr, &rec[6], &rec[7]);
            }
        }
    }
    if (!ok) {  // "no inlier" record: every comparison of the scoring kernels fails
        for (int k = 0; k < kModelStride; ++k) rec[k] = 0.0;
        if (KIND == 0) rec[4] = 0.0;  // num < 0 never holds
        if (KIND == 1) rec[3] = rec[4] = nan;
        if (KIND == 2) rec[6] = rec[7] = nan;
        for (int k = 0; k < kModelStride; ++k) par[k] = 0.0;
    }
    for (int k = 0; k < kModelStride; ++k) {
        score[(size_t)h * kModelStride + k] = rec[k];
        params[(size_t)h * kModelStride + k] = par[k];
    }
    valid[h] = ok ? 1 : 0;
    if (c32.out) {
        // fp32 record of the box tests, interleaved with the neighbour's: floats 2 k + (h & 1) of the pair's 24
        float cr[12];
        if (KIND == 0) plane_cull32_record(rec, ok, c32.origin, c32.radius, cull_max_abs, cr);
        else if (KIND == 1) sphere_cull32_record(rec, ok, c32.origin, c32.radius, cull_max_abs, cr);
        else cylinder_cull32_record(rec, ok, c32.origin, c32.radius, cull_max_abs, cr);
        float* dst = c32.out + (size_t)(h >> 1) * 24u + (h & 1u);
#pragma unroll
        for (int k = 0; k < 12; ++k) dst[2 * k] = cr[k];
    }
}

bool launch_minimal_fit(int kind, const CloudView& c, const uint32_t* samples, uint32_t h_count,
                        uint32_t h_pad, double thr, double* score, double* params, uint8_t* valid,
                        hipStream_t s, uint32_t* zero_u32, uint32_t* zero_one, const LeadPrep* lead, double cull_max_abs,
                        const Cull32Out* cull32, const PoisonJob* poison, uint32_t* zero_u32b) {
    if (h_pad == 0) return false;
    const uint32_t fit_blocks = (h_pad + 63) / 64;
    const dim3 g(fit_blocks + (kind == 0 && poison ? poison->n_tiles : 0u)), b(64);
    LeadPrep lp;
    if (lead) lp = *lead;
    Cull32Out c32;
    if (cull32) c32 = *cull32;
    PoisonJob pj;
    if (kind == 0 && poison) pj = *poison;
    if (kind == 0)
        minimal_fit_k<0><<<g, b, 0, s>>>(c, samples, h_count, h_pad, thr, score, params, valid, zero_u32, zero_u32b, zero_one, lp, cull_max_abs, c32, pj, fit_blocks);
    else if (kind == 1)
        minimal_fit_k<1><<<g, b, 0, s>>>(c, samples, h_count, h_pad, thr, score, params, valid, zero_u32, zero_u32b, zero_one, lp, cull_max_abs, c32, pj, fit_blocks);
    else
        minimal_fit_k<2><<<g, b, 0, s>>>(c, samples, h_count, h_pad, thr, score, params, valid, zero_u32, zero_u32b, zero_one, lp, cull_max_abs, c32, pj, fit_blocks);
    return true;
}

// ------------------------------------------------------------------------------------------------
// K2  inlier counting: (points of one tile, held in VGPRs) x (hypotheses streamed through SGPRs)
// ------------------------------------------------------------------------------------------------
// Workgroup = 256 threads = 4 waves; wave w owns rows of 64 consecutive points, kScoreP rows, so
// every global load is a fully coalesced 512-B row.  For each hypothesis the wave-uniform record
// is fetched with scalar loads, each of the P rows costs 6/8/20 fp64 VALU ops + compare(s), the
// 64-bit compare mask is popcounted on the scalar unit.  The count of hypothesis (hb + j) is
// parked in lane j of `acc` (one v_cndmask), and every 64 hypotheses the four waves combine through
// LDS and store one coalesced 256-B row of partial counts.
template <int KIND>
__global__ __launch_bounds__(kScoreBlock) void score_k(const double* __restrict__ xs,
                                                        const double* __restrict__ ys,
                                                        const double* __restrict__ zs,
                                                        const double* __restrict__ score,
                                                        uint32_t h_pad, uint32_t h_per_split,
                                                        uint32_t h_end,
                                                        uint32_t* __restrict__ partial) {
    __shared__ uint32_t red[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const size_t base = (size_t)blockIdx.x * kScoreTile + (size_t)wave * (64 * kScoreP) + lane;
    double x[kScoreP], y[kScoreP], z[kScoreP];
#pragma unroll
    for (int j = 0; j < kScoreP; ++j) {
        x[j] = xs[base + 64 * j];
        y[j] = ys[base + 64 * j];
        z[j] = zs[base + 64 * j];
    }
    const uint32_t h0 = blockIdx.y * h_per_split;
    const uint32_t h1 = min(h0 + h_per_split, h_end);  // the last split may be shorter
    // Software prefetch of the next hypothesis record: the scalar loads for hypothesis h+1 are
    // issued before the VALU work of hypothesis h (the score buffer carries one spare record).
    double rec[kModelStride];
    {
        const double* __restrict__ m = score + (size_t)h0 * kModelStride;
#pragma unroll
        for (int k = 0; k < kModelStride; ++k) rec[k] = m[k];
    }
    for (uint32_t hb = h0; hb < h1; hb += 64) {
        uint32_t acc = 0;
        for (uint32_t hh = 0; hh < 64; ++hh) {
            const double* __restrict__ mn = score + (size_t)(hb + hh + 1) * kModelStride;
            double nxt[kModelStride];
            constexpr int kUsed = KIND == 2 ? 8 : 5;
#pragma unroll
            for (int k = 0; k < kUsed; ++k) nxt[k] = mn[k];
            uint32_t cnt = 0;
            if (KIND == 0) {
                const double a = rec[0], b = rec[1], c = rec[2], d = rec[3], T = rec[4];
#pragma unroll
                for (int j = 0; j < kScoreP; ++j) {
                    const double num = plane_num(a, b, c, d, x[j], y[j], z[j]);
                    cnt += (uint32_t)__popcll(__ballot(num < T));
                }
            } else if (KIND == 1) {
                const double cx = rec[0], cy = rec[1], cz = rec[2], lo = rec[3], hi = rec[4];
#pragma unroll
                for (int j = 0; j < kScoreP; ++j) {
                    const double sv = sphere_s(cx, cy, cz, x[j], y[j], z[j]);
                    cnt += (uint32_t)__popcll(__ballot(sv >= lo) & __ballot(sv <= hi));  // two v_cmp + s_and_b64
                }
            } else {
                const double cx = rec[0], cy = rec[1], cz = rec[2], rx = rec[3], ry = rec[4],
                             rz = rec[5];
                const double lo = rec[6], hi = rec[7];
#pragma unroll
                for (int j = 0; j < kScoreP; ++j) {
                    const double tv = line_t(cx, cy, cz, rx, ry, rz, x[j], y[j], z[j]);
                    cnt += (uint32_t)__popcll(__ballot(tv >= lo) & __ballot(tv <= hi));
                }
            }
            acc = ((uint32_t)lane == hh) ? cnt : acc;  // lane hh keeps the count of hypothesis hb + hh
#pragma unroll
            for (int k = 0; k < kUsed; ++k) rec[k] = nxt[k];
        }
        red[wave][lane] = acc;
        __syncthreads();
        if (wave == 0)
            partial[(size_t)blockIdx.x * h_pad + hb + lane] =
                (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
        __syncthreads();
    }
}

void launch_score(int kind, const CloudView& c, const double* score, uint32_t h_pad,
                  uint32_t h_splits, uint32_t* partial, hipStream_t s) {
    if (h_pad == 0 || c.n_pad == 0) return;
    // every split takes ceil(groups / splits) groups of 64 hypotheses; the last one may be shorter
    const uint32_t groups = h_pad / 64;
    const uint32_t gps = (groups + h_splits - 1) / h_splits;
    const uint32_t splits = (groups + gps - 1) / gps;
    const dim3 g(c.n_pad / kScoreTile, splits), b(kScoreBlock);
    const uint32_t hps = gps * 64;
    if (kind == 0)
        score_k<0><<<g, b, 0, s>>>(c.x, c.y, c.z, score, h_pad, hps, h_pad, partial);
    else if (kind == 1)
        score_k<1><<<g, b, 0, s>>>(c.x, c.y, c.z, score, h_pad, hps, h_pad, partial);
    else
        score_k<2><<<g, b, 0, s>>>(c.x, c.y, c.z, score, h_pad, hps, h_pad, partial);
}

// counts[h] += sum over a group of tiles.  Integer atomics: order-independent, exact.
constexpr int kReduceTilesPerBlock = 64;
__global__ __launch_bounds__(256) void reduce_partials_k(const uint32_t* __restrict__ partial,
                                                          uint32_t n_tiles, uint32_t h_pad,
                                                          uint32_t* __restrict__ counts) {
    __shared__ uint32_t red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t h = blockIdx.x * 64u + lane;
    const uint32_t t0 = blockIdx.y * kReduceTilesPerBlock;
    const uint32_t t1 = min(n_tiles, t0 + kReduceTilesPerBlock);
    uint32_t acc = 0;
    for (uint32_t t = t0 + wave; t < t1; t += 4) acc += partial[(size_t)t * h_pad + h];
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0) {
        const uint32_t v = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
        if (v) atomicAdd(&counts[h], v);
    }
}

void launch_reduce_partials(const uint32_t* partial, uint32_t n_tiles, uint32_t h_pad,
                            uint32_t* counts, hipStream_t s) {
    if (h_pad == 0 || n_tiles == 0) return;
    const dim3 g(h_pad / 64, (n_tiles + kReduceTilesPerBlock - 1) / kReduceTilesPerBlock), b(256);
    reduce_partials_k<<<g, b, 0, s>>>(partial, n_tiles, h_pad, counts);
}

// ------------------------------------------------------------------------------------------------
// K4  ordered compaction with the reference distance (RefineModel, tie-break error, segmentation)
// ------------------------------------------------------------------------------------------------
template <int NV>
__device__ __forceinline__ void block_tree_reduce(double (&acc)[NV], double* sm /* NV x 256 */) {
    for (int k = 0; k < NV; ++k) sm[k * 256 + threadIdx.x] = acc[k];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            for (int k = 0; k < NV; ++k) sm[k * 256 + threadIdx.x] += sm[k * 256 + threadIdx.x + off];
        __syncthreads();
    }
}

template <int KIND>
__device__ __forceinline__ double ref_distance(const double* m, double x, double y, double z) {
    if (KIND == 0) return plane_distance(m, x, y, z);
    if (KIND == 1) return sphere_distance(m, x, y, z);
    return cylinder_distance(m, x, y, z);
}

// SUMS (RefineModel of a plane / sphere fit): the same pass also accumulates, over the INLIERS, the raw moments
// GeneralFit needs about a provisional centre c0 taken from the model record (slots 4..6: the plane hypothesis' first
// sample point, the centroid of the sphere hypothesis' four) -- s = p - c0:
//   [0..2] sum s   [3..8] sum s s^T (xx,xy,xz,yy,yz,zz)   [9..11] sum s |s|^2 (sphere)
// one 16-double partial per workgroup (fixed tree: deterministic); scan_blocks_k folds the partials.  c0 lies
// among the inliers (a sample point is an inlier of its own minimal model), so the shift to the true mean (host, moments_about_mean,
// m3d_generalfit_fp.hpp) cancels at most a few bits -- a sphere's minimal CENTRE would not do: it lies a radius away
// from a cap of inliers, and the shift would cancel by (radius / extent)^3.  This
// replaces two gather passes over the inlier list (ransac.h:170-188, 302-316 read the points once more).
template <int KIND, bool SUMS>
__global__ __launch_bounds__(256) void compact_count_k(CloudView c, const double* __restrict__ model,
                                                        double thr, int invert,
                                                        uint32_t* __restrict__ block_counts,
                                                        double* __restrict__ model_copy,
                                                        double* __restrict__ moment_partial,
                                                        uint64_t* __restrict__ mask_host = nullptr,
                                                        uint32_t* __restrict__ counts_host = nullptr) {
    __shared__ uint32_t wsum[4];
    __shared__ unsigned long long wmask[kCompactTile / 64];
    double m[kModelStride];
    for (int k = 0; k < kModelStride; ++k) m[k] = model[k];
    // the model record (8 doubles) also goes where the caller wants a copy (pinned host memory): no copy command
    if (model_copy && blockIdx.x == 0 && threadIdx.x < kModelStride) model_copy[threadIdx.x] = model[threadIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t cnt = 0;
    const uint32_t base = blockIdx.x * kCompactTile;
    constexpr int NV = KIND == 1 ? 12 : 9;
    double acc[NV];
    for (int k = 0; k < NV; ++k) acc[k] = 0.0;
    const double c0x = m[4], c0y = m[5], c0z = m[6];
    for (int r = 0; r < kCompactTile / 256; ++r) {
        const uint32_t i = base + r * 256 + threadIdx.x;
        bool f = false;
        if (i < c.n) {
            const double px = c.x[i], py = c.y[i], pz = c.z[i];
            const double d = ref_distance<KIND>(m, px, py, pz);
            // invert 1: the points a removal keeps (not inliers); 2: ... of the SORTED copy, whose dead points (x = NaN:
            // poison_plane_inliers_k) go as well -- it holds no other non-finite point (grid_count_k leaves them out)
            f = (d < thr) != (invert != 0) && (invert != 2 || px == px);
            if (SUMS && f) {
                const double sx = px - c0x, sy = py - c0y, sz = pz - c0z;
                acc[0] += sx;
                acc[1] += sy;
                acc[2] += sz;
                acc[3] += sx * sx;
                acc[4] += sx * sy;
                acc[5] += sx * sz;
                acc[6] += sy * sy;
                acc[7] += sy * sz;
                acc[8] += sz * sz;
                if (KIND == 1) {
                    const double q = (sx * sx + sy * sy) + sz * sz;
                    acc[9] += sx * q;
                    acc[10] += sy * q;
                    acc[11] += sz * q;
                }
            }
        }
        const unsigned long long b = __ballot(f);
        cnt += (uint32_t)__popcll(b);
        if (lane == 0) wmask[r * 4 + wave] = b;   // word (i / 64) of the tile: creation order
    }
    if (lane == 0) wsum[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t mine = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        block_counts[blockIdx.x] = mine;
        // (m3d_config.mask_early: the tile's count goes to the host beside its mask row -- the expansion needs both and nothing else)
        if (counts_host) counts_host[blockIdx.x] = mine;
    }
    // the tile's 32 mask words as ONE 256-byte store of 32 consecutive lanes (a store per wave row would cross the host link
    // as a write of its own); the buffer holds whole tiles: words past n are zero
    if (mask_host && threadIdx.x < kCompactTile / 64)
        mask_host[(size_t)blockIdx.x * (kCompactTile / 64) + threadIdx.x] = wmask[threadIdx.x];
    if (SUMS) {
        __shared__ double sm[NV * 256];
        __syncthreads();
        block_tree_reduce<NV>(acc, sm);
        if (threadIdx.x < 12) moment_partial[(size_t)blockIdx.x * 16 + threadIdx.x] = (int)threadIdx.x < NV ? sm[threadIdx.x * 256] : 0.0;
    }
}

// exclusive scan of block_counts[0..nb) in place; total[0] = sum
// moment_partial != null: nb x 16 doubles from compact_count_k<.., true>; their sums (fixed order: thread t takes blocks
// t, t + 1024, ..., then a 1024-leaf tree) go to moment_out[0..11] -- device-visible host memory -- and
// moment_out[12] receives the total as a double.
__global__ __launch_bounds__(1024) void scan_blocks_k(uint32_t* __restrict__ v, uint32_t nb,
                                                       uint32_t* __restrict__ total,
                                                       const double* __restrict__ moment_partial,
                                                       double* __restrict__ moment_out,
                                                       uint32_t* __restrict__ total_host /* device-visible copy of total[0], or null */) {
    __shared__ uint32_t buf[1024];
    __shared__ uint32_t carry;
    __shared__ double msum[12 * 64];
    if (moment_partial) {   // block-uniform
        // 16 lanes-groups of 64 threads: thread (g, l) sums blocks l, l + 64, ... of value g (g < 12)
        const uint32_t g = threadIdx.x >> 6, l = threadIdx.x & 63;
        if (g < 12) {
            double a = 0.0;
            for (uint32_t b = l; b < nb; b += 64) a += moment_partial[(size_t)b * 16 + g];
            msum[g * 64 + l] = a;
        }
        __syncthreads();
        for (int off = 32; off > 0; off >>= 1) {
            if (g < 12 && (int)l < off) msum[g * 64 + l] += msum[g * 64 + l + off];
            __syncthreads();
        }
        if (threadIdx.x < 12) moment_out[threadIdx.x] = msum[threadIdx.x * 64];
    }
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < nb; b0 += 1024) {
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t mine = i < nb ? v[i] : 0;
        buf[threadIdx.x] = mine;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const uint32_t t = threadIdx.x >= (uint32_t)off ? buf[threadIdx.x - off] : 0;
            __syncthreads();
            buf[threadIdx.x] += t;
            __syncthreads();
        }
        const uint32_t incl = buf[threadIdx.x];
        const uint32_t c0 = carry;
        if (i < nb) v[i] = c0 + incl - mine;
        __syncthreads();
        if (threadIdx.x == 1023) carry = c0 + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        total[0] = carry;
        if (total_host) total_host[0] = carry;
        if (moment_out) moment_out[12] = (double)carry;
    }
}

void launch_scan_blocks(uint32_t* v, uint32_t nb, uint32_t* total, hipStream_t s) {
    scan_blocks_k<<<1, 1024, 0, s>>>(v, nb, total, nullptr, nullptr, nullptr);
}

// what scan_blocks_k used to deliver between the counting and the writing pass, now produced by compact_write_k itself
struct CompactTail {
    uint32_t* total = nullptr;         // device: [0] = number of flagged points
    uint32_t* total_host = nullptr;    // device-visible host copy (may be null)
    const double* moment_partial = nullptr;   // compact_count_k<.., true>'s per-workgroup partials (may be null)
    double* moment_out = nullptr;      // ... folded: [0..11], [12] = the total as a double
    uint32_t nb = 0;
};
__device__ __forceinline__ void compact_tail_total(const CompactTail& t, uint32_t total) {
    if (t.total) t.total[0] = total;
    if (t.total_host) t.total_host[0] = total;
    if (t.moment_out) t.moment_out[12] = (double)total;
}

// RefineModel's moment partials folded by ONE workgroup of 256 threads (what scan_blocks_k did: thread (g, l) sums workgroups
// l, l + 64, ... of value g, then a 64-leaf tree -- the same order, the same sums)
__device__ __forceinline__ void fold_moment_partials(const CompactTail& tail) {
    __shared__ double msum[4 * 64];
    const uint32_t gq = threadIdx.x >> 6, l = threadIdx.x & 63u;
    for (uint32_t g0 = 0; g0 < 12u; g0 += 4u) {
        const uint32_t g = g0 + gq;
        double a = 0.0;
        // (unrolled: the loads of a lane go out together -- the sum keeps its order; in the mask form this fold is on the
        // step's critical path, a chain of dependent loads would cost ~1 us per 64 workgroups)
#pragma unroll 8
        for (uint32_t b = l; b < tail.nb; b += 64u) a += tail.moment_partial[(size_t)b * 16 + g];
        msum[gq * 64 + l] = a;
        __syncthreads();
        for (int off = 32; off > 0; off >>= 1) {
            if ((int)l < off) msum[gq * 64 + l] += msum[gq * 64 + l + off];
            __syncthreads();
        }
        if (l == 0) tail.moment_out[g] = msum[gq * 64];
        __syncthreads();
    }
}

// The writing pass: `slots` holds compact_count_k's counts, one per tile of kCompactTile points.  (The two passes as ONE launch --
// counts published and awaited inside it -- were measured slower and removed: profiles/r04_compact_one_pass.txt.)
template <int KIND, int MODE>
__global__ __launch_bounds__(256) void compact_write_k(
    CloudView c, const double* __restrict__ model, double thr, const uint32_t* __restrict__ orig,
    uint32_t* __restrict__ slots, uint64_t* __restrict__ out_idx,
    double* __restrict__ out_dist, double* __restrict__ ox, double* __restrict__ oy,
    double* __restrict__ oz, uint32_t* __restrict__ oorig, uint32_t n_pad_cap,
    uint64_t* __restrict__ out_idx_host /* MODE 0 / 4: the caller's page-locked index list, written as well (may be null) */,
    CompactTail tail) {
    __shared__ uint32_t wsum[4];
    const uint32_t tile = blockIdx.x;
    constexpr int NM = 7;
    double m[NM];
    for (int k = 0; k < NM; ++k) m[k] = model[k];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // workgroup 0 also folds RefineModel's moment partials
    if (tail.moment_partial && blockIdx.x == 0) fold_moment_partials(tail);   // (workgroup-uniform)
    const uint32_t base = tile * kCompactTile;
    // All of the workgroup's rows are loaded and classified FIRST (8 rows x 3 coordinates in flight per thread), the
    // per-row wave counts meet in LDS behind ONE barrier, then every row is written.  (A barrier per row serialised
    // eight load -> ballot -> store round trips: mode 4 ran at 2.3 TB/s, 23 us per segmentation round on 1 M points.)
    constexpr int R = kCompactTile / 256;
    __shared__ uint32_t wf[R][4], wg[R][4];
    double px[R], py[R], pz[R], dd[MODE == 1 ? R : 1];
    uint32_t og[R];
    unsigned long long bf[R], bg[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t i = base + r * 256 + threadIdx.x;
        const bool in = i < c.n;
        px[r] = in ? c.x[i] : 0.0;
        py[r] = in ? c.y[i] : 0.0;
        pz[r] = in ? c.z[i] : 0.0;
        og[r] = (MODE == 0 || MODE == 2 || MODE == 4) ? (in && orig ? orig[i] : i) : 0u;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t i = base + r * 256 + threadIdx.x;
        const bool in = i < c.n;
        const double d = ref_distance<KIND>(m, px[r], py[r], pz[r]);
        if (MODE == 1) dd[r] = d;
        const bool inl = in && d < thr;
        // f: what modes 0 / 1 / 4 list (the inliers) resp. what modes 2 / 3 keep (the rest); g (mode 4): the rest
        // (mode 3, the sorted copy: its dead points -- x = NaN, poison_plane_inliers_k -- are dropped with the inliers)
        const bool f = MODE == 3 ? (in && !inl && px[r] == px[r]) : (MODE == 2 ? (in && !inl) : inl);
        bf[r] = __ballot(f);
        if (MODE == 4) bg[r] = __ballot(in && !inl);
        if (lane == 0) {
            wf[r][wave] = (uint32_t)__popcll(bf[r]);
            if (MODE == 4) wg[r][wave] = (uint32_t)__popcll(bg[r]);
        }
    }
    __syncthreads();
    // This workgroup's offset = the counts of the tiles below it, summed here: a few hundred loads per workgroup, all
    // workgroups at once, against a one-workgroup scan kernel and its launch gap (7 us) between two passes.
    uint32_t row_base;
    {
        uint32_t part = 0;
        for (uint32_t i = threadIdx.x; i < tile; i += 256u) part += slots[i];
        part = wave_sum(part);
        if (lane == 0) wsum[wave] = part;
        __syncthreads();
        row_base = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t rest_base = base - row_base;   // (mode 4: every workgroup before this one holds kCompactTile points of the cloud)
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint32_t woff = 0, woff2 = 0;
        for (int w = 0; w < wave; ++w) {
            woff += wf[r][w];
            if (MODE == 4) woff2 += wg[r][w];
        }
        if ((bf[r] >> lane) & 1ull) {
            const uint32_t pos = row_base + woff + (uint32_t)__popcll(bf[r] & below);
            if (MODE == 0 || MODE == 4) {
                if (out_idx) out_idx[pos] = (uint64_t)og[r];
                if (out_idx_host) out_idx_host[pos] = (uint64_t)og[r];   // 512-B bursts per wave row straight over the host link
            }
            if (MODE == 1) out_dist[pos] = dd[r];
            if (MODE == 2 || MODE == 3) {
                ox[pos] = px[r];
                oy[pos] = py[r];
                oz[pos] = pz[r];
                if (MODE == 2) oorig[pos] = og[r];
            }
        }
        if (MODE == 4 && ((bg[r] >> lane) & 1ull)) {
            const uint32_t pos = rest_base + woff2 + (uint32_t)__popcll(bg[r] & below);
            ox[pos] = px[r];
            oy[pos] = py[r];
            oz[pos] = pz[r];
            oorig[pos] = og[r];
        }
        row_base += (wf[r][0] + wf[r][1]) + (wf[r][2] + wf[r][3]);
        if (MODE == 4) rest_base += (wg[r][0] + wg[r][1]) + (wg[r][2] + wg[r][3]);
    }
    if (tile == gridDim.x - 1 && threadIdx.x == 0) compact_tail_total(tail, row_base);   // (the last tile ends with the total)
    // NaN padding of the freshly compacted SoA cloud, [n, n_pad): the last tile ends with row_base / rest_base = n
    if ((MODE == 2 || MODE == 3 || MODE == 4) && tile == gridDim.x - 1) {
        const uint32_t n = MODE == 4 ? rest_base : row_base;
        const uint32_t n_pad = min(n_pad_cap, (n + kScoreTile - 1) / kScoreTile * kScoreTile);
        const double nan = u2f(0x7FF8000000000000ull);
        for (uint32_t i = n + threadIdx.x; i < n_pad; i += 256u) {
            ox[i] = nan;
            oy[i] = nan;
            oz[i] = nan;
        }
    }
}

// The mask form's second launch (one workgroup): what compact_write_k's workgroup 0 and last tile delivered -- the folded
// moment partials (fold_moment_partials: the same order, the same sums) and the total -- plus the tile counts, copied to the
// host as one contiguous block (counts_host; null: compact_count_k has stored them itself).
// ready_word (page-locked, may be null): receives done_seq FIRST -- the launch in front of this one has put the mask and the
// tile counts into host memory, and that is all the expansion reads: the host writes the list under the fold below.  The order
// is the kernel boundary's (the mask belongs to the launch before, the word to this one), nothing inside a launch.
// done_word (page-locked, may be null): receives done_seq last, behind a system-scope fence -- the end of the compaction.
__global__ __launch_bounds__(256) void compact_mask_tail_k(const uint32_t* __restrict__ block_counts, CompactTail tail,
                                                            uint32_t* __restrict__ counts_host, uint32_t* ready_word,
                                                            uint32_t* done_word, uint32_t done_seq) {
    __shared__ uint32_t wsum[4];
    if (ready_word && threadIdx.x == 0) __hip_atomic_store(ready_word, done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t part = 0;
    for (uint32_t i = threadIdx.x; i < tail.nb; i += 256u) {
        const uint32_t v = block_counts[i];
        if (counts_host) counts_host[i] = v;
        part += v;
    }
    part = wave_sum(part);
    if (lane == 0) wsum[wave] = part;
    if (tail.moment_partial) fold_moment_partials(tail);   // (ends with a barrier)
    else __syncthreads();
    if (threadIdx.x == 0) compact_tail_total(tail, (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
    if (done_word) {
        __threadfence_system();   // (every thread: its counts, and the moments of the lanes that stored them)
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(done_word, done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

template <int KIND>
static void launch_compact_kind(const CloudView& c, const double* model, double thr, int mode,
                                const uint32_t* orig, uint64_t* out_idx, double* out_dist,
                                double* ox, double* oy, double* oz, uint32_t* oorig,
                                uint32_t n_pad_out, uint32_t* block_counts, uint32_t* total,
                                hipStream_t s, double* model_copy, double* moment_partial, double* moment_out,
                                uint64_t* out_idx_host, uint32_t* total_host, const PartitionOut* part,
                                uint64_t* mask_host, uint32_t* counts_host, uint32_t* done_word, uint32_t done_seq,
                                uint32_t* ready_word) {
    const uint32_t nb = (c.n + kCompactTile - 1) / kCompactTile;
    if (nb == 0) {
        (void)hipMemsetAsync(total, 0, sizeof(uint32_t), s);
        if (total_host) (void)hipMemcpyAsync(total_host, total, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (model_copy) (void)hipMemcpyAsync(model_copy, model, sizeof(double) * kModelStride, hipMemcpyDeviceToHost, s);
        if (moment_out) (void)hipMemsetAsync(moment_out, 0, sizeof(double) * 13, s);
        return;
    }
    const bool sums = moment_partial && moment_out && mode == 0 && KIND != 2;
    if (mask_host && counts_host && sums && !orig && !part) {
        // the mask form: no list is written anywhere -- the host expands the mask (m3d_mask_expand.hpp)
        // (ready_word: the counting launch stores the tile counts itself and the tail announces them before anything else)
        compact_count_k<KIND == 2 ? 0 : KIND, true><<<nb, 256, 0, s>>>(c, model, thr, 0, block_counts, model_copy, moment_partial,
                                                                       mask_host, ready_word ? counts_host : nullptr);
        CompactTail tail;
        tail.total = total;
        tail.total_host = total_host;
        tail.moment_partial = moment_partial;
        tail.moment_out = moment_out;
        tail.nb = nb;
        compact_mask_tail_k<<<1, 256, 0, s>>>(block_counts, tail, ready_word ? nullptr : counts_host, ready_word, done_word, done_seq);
        return;
    }
    if (sums)
        compact_count_k<KIND == 2 ? 0 : KIND, true><<<nb, 256, 0, s>>>(c, model, thr, 0, block_counts, model_copy, moment_partial);
    else
        compact_count_k<KIND, false><<<nb, 256, 0, s>>>(c, model, thr, mode == 3 ? 2 : (mode >= 2 ? 1 : 0), block_counts, model_copy, nullptr);
    CompactTail tail;
    tail.total = total;
    tail.total_host = total_host;
    tail.moment_partial = sums ? moment_partial : nullptr;
    tail.moment_out = sums ? moment_out : nullptr;
    tail.nb = nb;
    const PartitionOut none;
    const PartitionOut& po = part ? *part : none;
    if (mode == 0 && part && orig)
        compact_write_k<KIND, 4><<<nb, 256, 0, s>>>(c, model, thr, orig, block_counts, out_idx, nullptr, po.ox, po.oy, po.oz, po.oorig,
                                                    po.n_pad_cap, out_idx_host, tail);
    else if (mode == 0)
        compact_write_k<KIND, 0><<<nb, 256, 0, s>>>(c, model, thr, orig, block_counts, out_idx, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                    0u, out_idx_host, tail);
    else if (mode == 1)
        compact_write_k<KIND, 1><<<nb, 256, 0, s>>>(c, model, thr, orig, block_counts, nullptr, out_dist, nullptr, nullptr, nullptr, nullptr,
                                                    0u, nullptr, tail);
    else if (mode == 2)
        compact_write_k<KIND, 2><<<nb, 256, 0, s>>>(c, model, thr, orig, block_counts, nullptr, nullptr, ox, oy, oz, oorig, n_pad_out,
                                                    nullptr, tail);
    else
        compact_write_k<KIND, 3><<<nb, 256, 0, s>>>(c, model, thr, nullptr, block_counts, nullptr, nullptr, ox, oy, oz, nullptr, n_pad_out,
                                                    nullptr, tail);
}

void launch_compact(int kind, const CloudView& c, const double* model, double thr, int mode,
                    const uint32_t* orig, uint64_t* out_idx, double* out_dist, double* ox,
                    double* oy, double* oz, uint32_t* oorig, uint32_t n_pad_out,
                    uint32_t* block_counts, uint32_t* total, hipStream_t s, double* model_copy,
                    double* moment_partial, double* moment_out, uint64_t* out_idx_host, uint32_t* total_host,
                    const PartitionOut* part, uint64_t* mask_host, uint32_t* counts_host, uint32_t* done_word,
                    uint32_t done_seq, uint32_t* ready_word) {
    if (kind == 0)
        launch_compact_kind<0>(c, model, thr, mode, orig, out_idx, out_dist, ox, oy, oz, oorig, n_pad_out, block_counts, total, s,
                               model_copy, moment_partial, moment_out, out_idx_host, total_host, part, mask_host, counts_host, done_word, done_seq, ready_word);
    else if (kind == 1)
        launch_compact_kind<1>(c, model, thr, mode, orig, out_idx, out_dist, ox, oy, oz, oorig, n_pad_out, block_counts, total, s,
                               model_copy, moment_partial, moment_out, out_idx_host, total_host, part, mask_host, counts_host, done_word, done_seq, ready_word);
    else
        launch_compact_kind<2>(c, model, thr, mode, orig, out_idx, out_dist, ox, oy, oz, oorig, n_pad_out, block_counts, total, s,
                               model_copy, nullptr, nullptr, out_idx_host, total_host, part, nullptr, nullptr, nullptr, 0u, nullptr);
}

// cluster = pcd_copy->SelectByIndex(inliers) (iterative_plane_segmentation.cpp:32): the points of an index list, AoS, in
// list order.  On the host this is a strided walk over the whole input per big cluster (140 ms for the clusters of a
// 10 M-point room); on the device the resident SoA copy is gathered at HBM speed and shipped in one copy.
__global__ void gather_points_k(CloudView c, const uint64_t* __restrict__ idx, size_t total, double* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const uint64_t j = idx[i];
    out[3 * i] = c.x[j];
    out[3 * i + 1] = c.y[j];
    out[3 * i + 2] = c.z[j];
}
void launch_gather_points(const CloudView& c, const uint64_t* idx, size_t total, double* out, hipStream_t s) {
    if (total) gather_points_k<<<(uint32_t)((total + 255) / 256), 256, 0, s>>>(c, idx, total, out);
}

// EvaluateModel's `error += distance` in point order (ransac.h:637): a genuinely serial fp64 chain.
// One wave: each lane loads one value of the next 64 (coalesced, prefetched one tile ahead), the
// values are broadcast in order with v_readlane (independent of the chain) and EVERY lane performs
// the same 64 dependent v_add_f64 -- no divergence, no LDS, no barrier; the chain runs at the
// fp64 add latency.  Lanes past the end contribute +0.0, which leaves the (non-negative) sum as is.
__global__ __launch_bounds__(64) void serial_sum_k(const double* __restrict__ v,
                                                    const uint32_t* __restrict__ n_ptr,
                                                    double* __restrict__ out) {
    // blocks of 1024 values: coalesced loads (16 per lane, next block in flight), parked in LDS, then read
    // back in order with wave-uniform addresses (LDS broadcast, two values per ds_read_b128) while EVERY lane
    // runs the same dependent v_add_f64 chain.  Values past the end are +0.0 (the sums are non-negative).
    __shared__ double buf[2][1024];
    const uint32_t n = n_ptr[0];
    const uint32_t lane = threadIdx.x;
    double s = 0.0;
    double r[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t i = (uint32_t)j * 64u + lane;
        r[j] = i < n ? v[i] : 0.0;
    }
    int cur = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += 1024u) {
#pragma unroll
        for (int j = 0; j < 16; ++j) buf[cur][j * 64 + lane] = r[j];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < 16; ++j) {   // next block
            const uint32_t i = b0 + 1024u + (uint32_t)j * 64u + lane;
            r[j] = i < n ? v[i] : 0.0;
        }
        const double2* __restrict__ p = reinterpret_cast<const double2*>(buf[cur]);
        for (int k = 0; k < 512; k += 8) {
            double2 t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = p[k + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                s += t[u].x;
                s += t[u].y;
            }
        }
        cur ^= 1;
    }
    if (lane == 0) out[0] = s;
}

// Order-free (tree) sums of the inlier distances + inlier counts of ONE or TWO models in one pass over the cloud: the cheap
// first stage of the tie rule.  |tree - serial| <= 2 n u * sum for n non-negative terms, so a tie is decided from these
// sums whenever they differ by more than that bound (any summation order serves); serial_sum_k runs only otherwise.
// The workgroup that finishes last folds the per-workgroup partials and stores (count_a, sum_a, count_b, sum_b) into
// `out` -- device-visible HOST memory: no memset, no second kernel, no copy command (a tie used to cost two passes, two
// fills, two folding kernels and four copies: ~110 us of a 140 us segmentation round).
constexpr int kErrBlocks = 512;
template <int KIND, bool PAIR>
__global__ __launch_bounds__(256) void error_sum_k(CloudView c, const double* __restrict__ model_a,
                                                    const double* __restrict__ model_b, double thr,
                                                    double* __restrict__ partial /* kErrBlocks x 4 */,
                                                    uint32_t* __restrict__ ticket, double* __restrict__ out) {
    __shared__ double sm[4 * 256];
    __shared__ uint32_t s_last;
    double ma[7], mb[7];
    for (int k = 0; k < 7; ++k) {
        ma[k] = model_a[k];
        mb[k] = PAIR ? model_b[k] : 0.0;
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};   // (count_a, sum_a, count_b, sum_b): counts < 2^31 are exact in fp64
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < c.n; i += gridDim.x * 256u) {
        const double x = c.x[i], y = c.y[i], z = c.z[i];
        const double da = ref_distance<KIND>(ma, x, y, z);
        if (da < thr) {
            acc[0] += 1.0;
            acc[1] += da;
        }
        if (PAIR) {
            const double db = ref_distance<KIND>(mb, x, y, z);
            if (db < thr) {
                acc[2] += 1.0;
                acc[3] += db;
            }
        }
    }
    block_tree_reduce<4>(acc, sm);
    // (release / acquire at agent scope around the ticket: the partials cross L2s -- one per XCD -- on their way to the
    // last workgroup)
    if (threadIdx.x < 4) {
        partial[blockIdx.x * 4 + threadIdx.x] = sm[threadIdx.x * 256];
        __threadfence();
    }
    __syncthreads();
    if (threadIdx.x == 0)
        s_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
    __syncthreads();
    if (!s_last) return;   // (workgroup-uniform)
    __threadfence();
    for (int k = 0; k < 4; ++k) acc[k] = 0.0;
    for (uint32_t b = threadIdx.x; b < gridDim.x; b += 256u) {
        const double4 v = *reinterpret_cast<const double4*>(partial + b * 4);
        acc[0] += v.x;
        acc[1] += v.y;
        acc[2] += v.z;
        acc[3] += v.w;
    }
    __syncthreads();
    block_tree_reduce<4>(acc, sm);
    if (threadIdx.x < 4) out[threadIdx.x] = sm[threadIdx.x * 256];
    if (threadIdx.x == 0) *ticket = 0u;   // (ready for the next launch on this stream)
}

void launch_serial_sum(const double* v, const uint32_t* n, double* out, hipStream_t s) {
    serial_sum_k<<<1, 64, 0, s>>>(v, n, out);
}

// ------------------------------------------------------------------------------------------------
// K5/K6  GeneralFit sums: fixed-shape two-level tree (deterministic for a given inlier count)
// ------------------------------------------------------------------------------------------------
constexpr int kSumBlocks = 256;

__global__ __launch_bounds__(256) void sum_xyz_k(CloudView c, const uint64_t* __restrict__ idx,
                                                  uint32_t n, double* __restrict__ partial) {
    __shared__ double sm[3 * 256];
    double acc[3] = {0, 0, 0};
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < n; k += kSumBlocks * 256u) {
        const uint64_t i = idx[k];
        acc[0] += c.x[i];
        acc[1] += c.y[i];
        acc[2] += c.z[i];
    }
    block_tree_reduce<3>(acc, sm);
    if (threadIdx.x < 3) partial[blockIdx.x * 16 + threadIdx.x] = sm[threadIdx.x * 256];
}

// Second pass of the GeneralFit sums.  Every workgroup first folds the 256 x/y/z partials of sum_xyz_k itself
// (one fixed 256-leaf tree, block_tree_reduce: identical mean everywhere, no kernel in between), then accumulates its
// share of the centred moments.  `out` is device-visible HOST memory (pinned): the per-workgroup partials
// (out[block * 16 + k]) and, from workgroup 0, the three coordinate sums (out[kSumBlocks * 16 + k]) land there
// without a copy command; the host finishes the 256-leaf tree (general_fit_sums_finish, same order).
__global__ __launch_bounds__(256) void sum_moments_k(CloudView c, const uint64_t* __restrict__ idx,
                                                      uint32_t n,
                                                      const double* __restrict__ partial_xyz,
                                                      double* __restrict__ out) {
    __shared__ double sm[10 * 256];
    double s3[3];
    for (int k = 0; k < 3; ++k) s3[k] = partial_xyz[threadIdx.x * 16 + k];  // kSumBlocks == 256
    block_tree_reduce<3>(s3, sm);
    const double sx = sm[0], sy = sm[256], sz = sm[512];
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out[kSumBlocks * 16 + 0] = sx;
        out[kSumBlocks * 16 + 1] = sy;
        out[kSumBlocks * 16 + 2] = sz;
    }
    // mean /= double(num), ransac.h:176
    const double mx = sx / (double)n, my = sy / (double)n, mz = sz / (double)n;
    double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < n; k += kSumBlocks * 256u) {
        const uint64_t i = idx[k];
        const double r0 = c.x[i] - mx, r1 = c.y[i] - my, r2 = c.z[i] - mz;
        const double q = (r0 * r0 + r1 * r1) + r2 * r2;
        acc[0] += r0 * r0;
        acc[1] += r0 * r1;
        acc[2] += r0 * r2;
        acc[3] += r1 * r1;
        acc[4] += r1 * r2;
        acc[5] += r2 * r2;
        acc[6] += r0 * q;
        acc[7] += r1 * q;
        acc[8] += r2 * q;
        acc[9] += q;
    }
    block_tree_reduce<10>(acc, sm);
    if (threadIdx.x < 10) out[blockIdx.x * 16 + threadIdx.x] = sm[threadIdx.x * 256];
}


void launch_general_fit_sums(const CloudView& c, const uint64_t* idx, uint32_t n_idx, double* partial_dev,
                             double* out_host, hipStream_t s) {
    sum_xyz_k<<<kSumBlocks, 256, 0, s>>>(c, idx, n_idx, partial_dev);
    sum_moments_k<<<kSumBlocks, 256, 0, s>>>(c, idx, n_idx, partial_dev, out_host);
}

// sums[0..2] = sum of x, y, z; sums[4..13] = the ten centred moments: the last level of the fixed tree, on the host,
// in block_tree_reduce's order (bit-identical to the one-workgroup folding kernel it replaced)
void general_fit_sums_finish(const double* out_host, double* sums14) {
    for (int k = 0; k < 3; ++k) sums14[k] = out_host[kSumBlocks * 16 + k];
    sums14[3] = 0.0;
    double t[256];
    for (int k = 0; k < 10; ++k) {
        for (int b = 0; b < 256; ++b) t[b] = out_host[b * 16 + k];
        for (int off = 128; off > 0; off >>= 1)
            for (int b = 0; b < off; ++b) t[b] += t[b + off];
        sums14[4 + k] = t[0];
    }
}

void launch_error_sum(int kind, const CloudView& c, const double* model_a, const double* model_b, double thr,
                      double* partial, uint32_t* ticket, double* out_host, hipStream_t s) {
    const uint32_t g = std::max<uint32_t>(1u, std::min<uint32_t>((uint32_t)kErrBlocks, (c.n + 2047u) / 2048u));
#define M3D_ERR(K)                                                                                          \
    (model_b ? error_sum_k<K, true><<<g, 256, 0, s>>>(c, model_a, model_b, thr, partial, ticket, out_host) \
             : error_sum_k<K, false><<<g, 256, 0, s>>>(c, model_a, model_a, thr, partial, ticket, out_host))
    if (kind == 0) M3D_ERR(0);
    else if (kind == 1) M3D_ERR(1);
    else M3D_ERR(2);
#undef M3D_ERR
}

}  // namespace m3d

// ------------------------------------------------------------------------------------------------
// measurement probe (include/misc3d_amd_bench.h): what the chip sustains on the instruction mix the scoring kernels
// are bound by -- independent v_mul_f64 / v_add_f64 chains, no FMA, no memory -- at the clock it settles to under
// that load.  bench.py quotes the scoring kernel against the nominal 2.4 GHz peak (roofline.frac) and, beside it,
// against this measured rate.
// ------------------------------------------------------------------------------------------------
namespace m3d {
__global__ __launch_bounds__(256) void fp64_issue_probe_k(double* __restrict__ out, int iters, double seed) {
    double a[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = seed + (double)(threadIdx.x + k);
    const double m = 1.0000000001, c = 1e-9;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            a[k] = a[k] * m;   // v_mul_f64
            a[k] = a[k] + c;   // v_add_f64 (separately rounded: -ffp-contract=off)
        }
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += a[k];
    if (s == 12345.678) out[0] = s;   // keeps the chains alive, never true in practice
}
void launch_fp64_issue_probe(double* out, int blocks, int iters, hipStream_t st) {
    fp64_issue_probe_k<<<blocks, 256, 0, st>>>(out, iters, 1.0);
}
}  // namespace m3d
