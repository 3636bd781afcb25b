// m3d_fps.hip -- farthest point sampling (misc3d::preprocessing::FarthestPointSampling, src/filter.cpp:13-52) on gfx950.
//
// The reference's loop is serial and O(N S): for each sample one full pass that lowers dist[j] to the squared distance
// from the point selected last and picks the first index of the largest dist.  Both device paths reproduce it bit for bit:
// the per-point arithmetic is m3d_fps_fp.hpp's (the same sum3 association), and the argmax key is (dist desc, original
// index asc) over the points with dist > 0 -- when no distance is > 0 the previous index is emitted again.
//
// (a) fps_single_k: small clouds.  One workgroup of 1024 threads keeps up to 8 points per thread (coordinates and
//     distances) in VGPRs and runs all S steps in one launch: update, wave argmax through shuffles, the 16 wave winners
//     through LDS (double-buffered by step parity, so ONE __syncthreads per step), and every thread reduces the 16 itself.
// (b) fps_step_k: large clouds.  The finite points in Hilbert-sorted tiles of 512 with exact fp64 boxes and a record
//     (tmax, tidx) per tile; one launch per sample.  A wave skips a tile when fps_box_lb(box, s) >= tmax (exact: the
//     argument is in m3d_fps_fp.hpp), else it updates the tile's points and its record.  Every workgroup writes its best
//     record; the last one to draw the ticket (agent-scope release before, acquire after) reduces them, adds the constant
//     (+inf, lowest non-finite index) candidate, writes the sample and the selected point and resets the ticket.  Nothing
//     waits for another workgroup.
#include "m3d_fps.hpp"
#include "m3d_fps_fp.hpp"

namespace m3d {

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

// argmax of (d, i) over the 64 lanes of a wave (fps_better is a strict total order: every lane ends with the same pair)
__device__ __forceinline__ void wave_argmax(double& d, uint32_t& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(d, off, 64);
        const uint32_t oi = (uint32_t)__shfl_xor((int)i, off, 64);
        if (fps_better(od, oi, d, i)) {
            d = od;
            i = oi;
        }
    }
}

template <int PPT>
__global__ __launch_bounds__(kFpsSingleThreads) void fps_single_k(const double* __restrict__ aos, uint32_t n, uint32_t S,
                                                                  uint32_t* __restrict__ out) {
    constexpr int kWaves = kFpsSingleThreads / 64;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ double s_d[2][kWaves];
    __shared__ uint32_t s_i[2][kWaves];
    __shared__ double s_p[2][kWaves][3];
    double px[PPT], py[PPT], pz[PPT], dist[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const uint32_t j = (uint32_t)k * kFpsSingleThreads + tid;
        if (j < n) {
            px[k] = aos[3 * (size_t)j];
            py[k] = aos[3 * (size_t)j + 1];
            pz[k] = aos[3 * (size_t)j + 2];
            dist[k] = INFINITY;
        } else {   // padding: d is NaN and never lowers 0, and 0 is never a candidate
            px[k] = py[k] = pz[k] = NAN;
            dist[k] = 0.0;
        }
    }
    double sx = aos[0], sy = aos[1], sz = aos[2];
    uint32_t far = 0;
    for (uint32_t i = 0;; ++i) {
        if (tid == 0) out[i] = far;
        if (i + 1 >= S) break;   // (the reference's last pass changes nothing it returns)
        double bd = 0.0, bx = 0.0, by = 0.0, bz = 0.0;
        uint32_t bi = kNone;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const double d = fps_point_d(px[k], py[k], pz[k], sx, sy, sz);
            dist[k] = d < dist[k] ? d : dist[k];
            if (dist[k] > bd) {   // ascending index within the thread: the first maximum stays
                bd = dist[k];
                bi = (uint32_t)k * kFpsSingleThreads + tid;
                bx = px[k];
                by = py[k];
                bz = pz[k];
            }
        }
        double wd = bd;
        uint32_t wi = bi;
        wave_argmax(wd, wi);
        const int buf = (int)(i & 1u);
        if (lane == 0) {
            s_d[buf][wave] = wd;
            s_i[buf][wave] = wi;
        }
        if (wi != kNone && bi == wi) {   // the one lane that holds the wave's winner
            s_p[buf][wave][0] = bx;
            s_p[buf][wave][1] = by;
            s_p[buf][wave][2] = bz;
        }
        __syncthreads();   // (the other buffer is written next step: a thread still reading this one holds the next barrier)
        double gd = s_d[buf][0];
        uint32_t gi = s_i[buf][0];
        int gw = 0;
#pragma unroll
        for (int w = 1; w < kWaves; ++w)
            if (fps_better(s_d[buf][w], s_i[buf][w], gd, gi)) {
                gd = s_d[buf][w];
                gi = s_i[buf][w];
                gw = w;
            }
        if (gd > 0.0) {   // else no distance is > 0: the reference keeps farthest_index
            far = gi;
            sx = s_p[buf][gw][0];
            sy = s_p[buf][gw][1];
            sz = s_p[buf][gw][2];
        }
    }
}

__global__ __launch_bounds__(256) void fps_tiles_init_k(const double* __restrict__ sx, const double* __restrict__ sy,
                                                        const double* __restrict__ sz, const uint32_t* __restrict__ orig,
                                                        uint32_t n_tiles, double* __restrict__ dist, double* __restrict__ tiles) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (t >= n_tiles) return;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t tidx = kNone;
    for (int r = 0; r < kFpsTilePoints / 64; ++r) {
        const size_t j = (size_t)t * kFpsTilePoints + (size_t)r * 64 + lane;
        const uint32_t o = orig[j];
        const bool real = o != kNone;
        if (real) {
            const double p[3] = {sx[j], sy[j], sz[j]};
            for (int k = 0; k < 3; ++k) {   // (fmin / fmax drop a NaN coordinate: such a point never changes anything)
                lo[k] = fmin(lo[k], p[k]);
                hi[k] = fmax(hi[k], p[k]);
            }
            tidx = min(tidx, o);
        }
        dist[j] = real ? INFINITY : 0.0;
    }
    for (int off = 32; off > 0; off >>= 1) {
        for (int k = 0; k < 3; ++k) {
            lo[k] = fmin(lo[k], __shfl_xor(lo[k], off, 64));
            hi[k] = fmax(hi[k], __shfl_xor(hi[k], off, 64));
        }
        tidx = min(tidx, (uint32_t)__shfl_xor((int)tidx, off, 64));
    }
    if (lane == 0) {
        double* rec = tiles + (size_t)t * kFpsTileDoubles;
        for (int k = 0; k < 3; ++k) {
            rec[k] = lo[k];
            rec[3 + k] = hi[k];
        }
        rec[6] = tidx != kNone ? INFINITY : 0.0;
        reinterpret_cast<unsigned long long*>(rec)[7] = tidx;
    }
}

__global__ __launch_bounds__(256) void fps_step_k(const double* __restrict__ aos, const double* __restrict__ sx,
                                                  const double* __restrict__ sy, const double* __restrict__ sz,
                                                  const uint32_t* __restrict__ orig, uint32_t n_tiles, double* __restrict__ dist,
                                                  double* __restrict__ tiles, unsigned long long* __restrict__ wg_rec,
                                                  FpsState* __restrict__ state, uint32_t nf_idx, uint32_t* __restrict__ out,
                                                  uint32_t step, int prune) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    __shared__ double l_d[4];
    __shared__ uint32_t l_i[4], l_upd[4], l_last;
    const double s0 = state->sel[0], s1 = state->sel[1], s2 = state->sel[2];
    double bd = 0.0;
    uint32_t bi = kNone, upd = 0;
    for (uint32_t t = blockIdx.x * 4u + wave; t < n_tiles; t += gridDim.x * 4u) {
        double* rec = tiles + (size_t)t * kFpsTileDoubles;
        double tmax = rec[6];
        uint32_t tidx = (uint32_t)reinterpret_cast<const unsigned long long*>(rec)[7];
        // (wave-uniform: every lane reads the same record and computes the same bound)
        if (!(prune && fps_box_lb(rec, rec + 3, s0, s1, s2) >= tmax)) {
            double td = 0.0;
            uint32_t ti = kNone;
#pragma unroll
            for (int r = 0; r < kFpsTilePoints / 64; ++r) {
                const size_t j = (size_t)t * kFpsTilePoints + (size_t)r * 64 + lane;
                const double d = fps_point_d(sx[j], sy[j], sz[j], s0, s1, s2);
                double dj = dist[j];
                dj = d < dj ? d : dj;
                dist[j] = dj;
                const uint32_t o = orig[j];
                if (fps_better(dj, o, td, ti)) {
                    td = dj;
                    ti = o;
                }
            }
            wave_argmax(td, ti);
            tmax = td;
            tidx = ti;
            if (lane == 0) {
                rec[6] = td;
                reinterpret_cast<unsigned long long*>(rec)[7] = ti;
            }
            ++upd;
        }
        if (fps_better(tmax, tidx, bd, bi)) {
            bd = tmax;
            bi = tidx;
        }
    }
    if (lane == 0) {
        l_d[wave] = bd;
        l_i[wave] = bi;
        l_upd[wave] = upd;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double d = l_d[0];
        uint32_t ix = l_i[0], u = l_upd[0];
        for (int w = 1; w < 4; ++w) {
            u += l_upd[w];
            if (fps_better(l_d[w], l_i[w], d, ix)) {
                d = l_d[w];
                ix = l_i[w];
            }
        }
        if (u) __hip_atomic_fetch_add(&state->tiles_updated, (unsigned long long)u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        wg_rec[2 * (size_t)blockIdx.x] = f2u(d);
        wg_rec[2 * (size_t)blockIdx.x + 1] = ix;
        // hand-off to the last arriver (cdna_hip_programming.md section 6, Guideline 16): release, drain, ticket
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t ticket = __hip_atomic_fetch_add(&state->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        l_last = ticket == gridDim.x - 1u ? 1u : 0u;
        if (l_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!l_last) return;
    double gd = 0.0;
    uint32_t gi = kNone;
    for (uint32_t g = threadIdx.x; g < gridDim.x; g += blockDim.x) {
        const double d = u2f(wg_rec[2 * (size_t)g]);
        const uint32_t ix = (uint32_t)wg_rec[2 * (size_t)g + 1];
        if (fps_better(d, ix, gd, gi)) {
            gd = d;
            gi = ix;
        }
    }
    if (threadIdx.x == 0 && nf_idx != kNone && fps_better(INFINITY, nf_idx, gd, gi)) {
        gd = INFINITY;
        gi = nf_idx;
    }
    wave_argmax(gd, gi);
    if (lane == 0) {   // (l_d / l_i were last read by thread 0 before the barrier above)
        l_d[wave] = gd;
        l_i[wave] = gi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (fps_better(l_d[w], l_i[w], gd, gi)) {
                gd = l_d[w];
                gi = l_i[w];
            }
        const uint32_t far = gd > 0.0 ? gi : state->farthest;   // no distance > 0: the reference keeps farthest_index
        out[step] = far;
        state->farthest = far;
        state->sel[0] = aos[3 * (size_t)far];
        state->sel[1] = aos[3 * (size_t)far + 1];
        state->sel[2] = aos[3 * (size_t)far + 2];
        state->ticket = 0u;
    }
}

}  // namespace

void launch_fps_single(const double* aos, uint32_t n, uint32_t S, uint32_t* out, hipStream_t st) {
    const uint32_t ppt = (n + kFpsSingleThreads - 1) / kFpsSingleThreads;
    if (ppt <= 1)
        fps_single_k<1><<<1, kFpsSingleThreads, 0, st>>>(aos, n, S, out);
    else if (ppt <= 2)
        fps_single_k<2><<<1, kFpsSingleThreads, 0, st>>>(aos, n, S, out);
    else if (ppt <= 4)
        fps_single_k<4><<<1, kFpsSingleThreads, 0, st>>>(aos, n, S, out);
    else
        fps_single_k<8><<<1, kFpsSingleThreads, 0, st>>>(aos, n, S, out);
}

void launch_fps_tiles_init(const double* sx, const double* sy, const double* sz, const uint32_t* orig, uint32_t n_tiles,
                           double* dist, double* tiles, hipStream_t st) {
    if (n_tiles) fps_tiles_init_k<<<(n_tiles + 3) / 4, 256, 0, st>>>(sx, sy, sz, orig, n_tiles, dist, tiles);
}

uint32_t fps_step_grid(uint32_t n_tiles) {
    const uint32_t g = (n_tiles + 3) / 4;
    return g < 1 ? 1 : (g > 1024 ? 1024 : g);
}

void launch_fps_step(const double* aos, const double* sx, const double* sy, const double* sz, const uint32_t* orig,
                     uint32_t n_tiles, double* dist, double* tiles, double* wg_rec, FpsState* state, uint32_t nf_idx,
                     uint32_t* out, uint32_t i, bool prune, hipStream_t st) {
    fps_step_k<<<fps_step_grid(n_tiles), 256, 0, st>>>(aos, sx, sy, sz, orig, n_tiles, dist, tiles,
                                                      reinterpret_cast<unsigned long long*>(wg_rec), state, nf_idx, out, i,
                                                      prune ? 1 : 0);
}

}  // namespace m3d
