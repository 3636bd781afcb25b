// m3d_ppf.hip -- the kernels of the PPF table (CalcHashTable, GenerateModelPCNeighbor) and of the vote (VotingAndGetPose,
// CalcLocalMaximum) for gfx950, in both voting modes.  Contract: include/misc3d_amd.h "PPF voting" and "PPF voting,
// EdgePoints mode"; arithmetic: m3d_ppf_fp.hpp.  Every output is
// an integer: counts by atomics, sets by atomic-or, lists put in order by a stable sort or by the host.
#include "m3d_ppf.hpp"
#include "m3d_wave.hpp"

#include <algorithm>

#pragma clang fp contract(off)

namespace m3d {

namespace {

__global__ void ppf_pair_keys_k(PpfModelView M, uint32_t* keys) {
    const unsigned long long pairs = (unsigned long long)M.n * M.n_e;
    for (unsigned long long p = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; p < pairs;
         p += (unsigned long long)gridDim.x * blockDim.x) {
        const uint32_t i = (uint32_t)(p / M.n_e), j = (uint32_t)(p % M.n_e);
        uint32_t key = M.table_size;
        int q[4], qa;
        if (!(M.same_set && i == j) &&
            ppf_pair_bins(M.T, M.pts + 3 * (size_t)i, M.nrm + 3 * (size_t)i, M.epts + 3 * (size_t)j, M.enrm + 3 * (size_t)j,
                          M.frames + 8 * (size_t)i, q, &qa))
            key = ppf_cell(M.T, q) | (uint32_t)qa << 24;
        keys[p] = key;
    }
}

// position t starts the cells (previous key, this key]; the last position also ends every cell behind its key
__global__ void ppf_cell_offsets_k(const uint32_t* keys, uint32_t pairs, uint32_t table_size, uint32_t* cell_off) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= pairs) return;
    const uint32_t cur = keys[t] & kPpfKeyCellMask;
    const uint32_t first = t ? (keys[t - 1] & kPpfKeyCellMask) + 1 : 0;
    for (uint32_t c = first; c <= cur && c <= table_size; ++c) cell_off[c] = t;
    if (t == pairs - 1)
        for (uint32_t c = cur + 1; c <= table_size; ++c) cell_off[c] = pairs;
}

__global__ void ppf_entries_k(const uint32_t* keys, const uint32_t* vals, uint32_t n_entries, uint32_t n_e, uint32_t table_size,
                              uint32_t* entries) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_entries) return;   // (the skipped pairs sort behind every cell)
    const uint32_t key = keys[t];
    if ((key & kPpfKeyCellMask) >= table_size) return;
    entries[t] = vals[t] / n_e | (key >> 24) << 16;
}

__global__ void ppf_nbr_count_k(const double* pts, uint32_t n, double r2, uint32_t* counts) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t c = 0;
    for (uint32_t j = 0; j < n; ++j) c += ppf_d2(pts + 3 * (size_t)i, pts + 3 * (size_t)j) < r2 ? 1u : 0u;
    counts[i] = c;
}

__global__ void ppf_nbr_fill_k(const double* pts, uint32_t n, double r2, const uint32_t* offsets, uint32_t* idx) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t at = offsets[i];
    const uint32_t end = offsets[i + 1];
    for (uint32_t j = 0; j < n && at < end; ++j)
        if (ppf_d2(pts + 3 * (size_t)i, pts + 3 * (size_t)j) < r2) idx[at++] = j;
}

// counter idx of the accumulator.  In device memory the counters were written by atomics, which act on L2: the read goes
// there too (an agent-scope load), past the CU's vector cache.
template <bool kLds>
__device__ __forceinline__ uint32_t acc_get(const uint32_t* acc, uint32_t idx) {
    const uint32_t w = kLds ? acc[idx >> 1] : __hip_atomic_load(&acc[idx >> 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (w >> (16 * (idx & 1))) & 0xFFFFu;
}

// One pass of a wave over its share of the scene for the reference point (p0, n0, frame): the neighbours that pass the
// filter, their spread cells, and per cell either the vote (kClear == false: the first arrival of (cell, alpha bin) adds
// the cell's entries to acc) or the reset of the cell's flag word (kClear == true, the same cells once more).
template <bool kClear>
__device__ __forceinline__ void ppf_scene_pass(const PpfVoteArgs& a, const double* p0, const double* n0, const double* frame,
                                               unsigned long long* flags, uint32_t* acc, int lane, uint32_t wave, uint32_t waves,
                                               unsigned long long* increments) {
    const PpfTables& T = a.M.T;
    const int spread = ppf_spread_count(T);
    const int A = T.alpha_num;
    for (uint32_t base = wave * 64; base < a.m; base += waves * 64) {
        const uint32_t j = base + (uint32_t)lane;
        int q[4] = {0, 0, 0, 0}, qa = 0;
        bool votes = false;
        if (j < a.m) {
            const double* p1 = a.spts + 3 * (size_t)j;
            const double* n1 = a.snrm + 3 * (size_t)j;
            const double d2 = ppf_d2(p0, p1);
            if (d2 < a.r2 && !ppf_pair_filtered(d2, n0, n1, a.dist_thresh, a.cos_thresh))
                votes = ppf_pair_bins(T, p0, n0, p1, n1, frame, q, &qa);
        }
        unsigned long long todo = __ballot(votes);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            int qs[4];
            for (int c = 0; c < 4; ++c) qs[c] = __shfl(q[c], src, 64);
            const int qas = __shfl(qa, src, 64);
            for (int sb = 0; sb < spread; sb += 64) {
                const int s = sb + lane;
                const int64_t cell = s < spread ? ppf_spread_cell(T, qs, s) : -1;
                uint32_t beg = 0, end = 0;
                bool first = false;
                if (cell >= 0) {
                    beg = a.M.cell_off[cell];
                    end = a.M.cell_off[cell + 1];
                    if (end > beg) {
                        if (kClear) {
                            atomicExch(&flags[cell], 0ull);   // (through L2, as the atomic-or)
                        } else {
                            const unsigned long long bit = 1ull << qas;
                            first = !(atomicOr(&flags[cell], bit) & bit);
                        }
                    }
                }
                if (kClear) continue;
                unsigned long long cells = __ballot(first);
                while (cells) {
                    const int l = __ffsll((long long)cells) - 1;
                    cells &= cells - 1;
                    const uint32_t b = (uint32_t)__shfl((int)beg, l, 64), e = (uint32_t)__shfl((int)end, l, 64);
                    for (uint32_t t = b + (uint32_t)lane; t < e; t += 64) {
                        const uint32_t ent = a.M.entries[t];
                        const uint32_t idx = (ent & 0xFFFFu) * (uint32_t)A + (uint32_t)ppf_alpha_index((int)(ent >> 16), qas, A);
                        atomicAdd(&acc[idx >> 1], 1u << (16 * (idx & 1)));
                    }
                    if (lane == 0) *increments += e - b;
                }
            }
        }
    }
}

template <bool kLds>
__global__ __launch_bounds__(kPpfVoteThreads) void ppf_vote_k(PpfVoteArgs a) {
    extern __shared__ uint32_t ppf_smem[];
    __shared__ uint32_t s_count, s_max;
    const uint32_t n = a.M.n;
    const int A = a.M.T.alpha_num;
    const uint32_t bm_words = (n + 31) / 32;
    uint32_t* cand = ppf_smem;                 // rows above 0.8 max
    uint32_t* max_flags = ppf_smem + bm_words;
    uint32_t* acc = kLds ? ppf_smem + 2 * bm_words : a.acc + (size_t)blockIdx.x * a.acc_words;
    unsigned long long* flags = a.flags + (size_t)blockIdx.x * a.M.table_size;
    uint32_t* rowinfo = a.rowinfo + (size_t)blockIdx.x * n;
    const uint32_t tid = threadIdx.x, threads = blockDim.x;
    const int lane = (int)(tid & 63);
    const uint32_t wave = tid >> 6, waves = threads >> 6;
    unsigned long long increments = 0, visited = 0;

    for (uint32_t r = blockIdx.x; r < a.n_ref; r += gridDim.x) {
        const uint32_t ri = a.ref[r];
        double p0[3], n0[3], frame[8];
        for (int c = 0; c < 3; ++c) {
            p0[c] = a.rpts[3 * (size_t)ri + c];
            n0[c] = a.rnrm[3 * (size_t)ri + c];
        }
        for (int c = 0; c < 8; ++c) frame[c] = a.sframes[8 * (size_t)r + c];
        if (tid == 0) {
            s_count = 0;
            s_max = 0;
        }
        __syncthreads();
        uint32_t mine = 0;
        for (uint32_t j = tid; j < a.m; j += threads) mine += ppf_d2(p0, a.spts + 3 * (size_t)j) < a.r2 ? 1u : 0u;
        mine = wave_sum(mine);
        if (lane == 0) atomicAdd(&s_count, mine);
        __syncthreads();
        const uint32_t searched = s_count;
        __syncthreads();   // (s_count is reset by the next round)
        if (tid == 0) visited += searched;
        if (!(searched > a.gate)) continue;   // (the same for every thread: the next round's barrier is reached by all)

        for (uint32_t w = tid; w < a.acc_words; w += threads) acc[w] = 0;
        for (uint32_t w = tid; w < bm_words; w += threads) {
            cand[w] = 0;
            max_flags[w] = 0xFFFFFFFFu;
        }
        __syncthreads();
        ppf_scene_pass<false>(a, p0, n0, frame, flags, acc, lane, wave, waves, &increments);
        __syncthreads();

        // CalcLocalMaximum: every row's best circular three-window (strict >: the first wins)
        uint32_t best_of_mine = 0;
        for (uint32_t i = tid; i < n; i += threads) {
            const uint32_t row = i * (uint32_t)A;
            uint32_t best = acc_get<kLds>(acc, row + A - 1) + acc_get<kLds>(acc, row) + acc_get<kLds>(acc, row + 1), col = 0;
            for (int c = 1; c < A - 1; ++c) {
                const uint32_t t = acc_get<kLds>(acc, row + c - 1) + acc_get<kLds>(acc, row + c) + acc_get<kLds>(acc, row + c + 1);
                if (t > best) {
                    best = t;
                    col = (uint32_t)c;
                }
            }
            const uint32_t t = acc_get<kLds>(acc, row + A - 2) + acc_get<kLds>(acc, row + A - 1) + acc_get<kLds>(acc, row);
            if (t > best) {
                best = t;
                col = (uint32_t)(A - 1);
            }
            rowinfo[i] = best << 6 | col;
            best_of_mine = max(best_of_mine, best);
        }
        best_of_mine = wave_max(best_of_mine);
        if (lane == 0) atomicMax(&s_max, best_of_mine);
        __syncthreads();
        const uint32_t max_votes = s_max;
        if (max_votes >= a.gate) {
            const uint32_t thr = (uint32_t)(unsigned long long)((double)max_votes * 0.8);
            for (uint32_t i = tid; i < n; i += threads)
                if ((rowinfo[i] >> 6) > thr) atomicOr(&cand[i >> 5], 1u << (i & 31));
            __syncthreads();
            if (tid == 0) {   // the suppression pass, rows ascending, serial over the rows above the threshold
                for (uint32_t w = 0; w < bm_words; ++w) {
                    uint32_t bits = cand[w];
                    while (bits) {
                        const uint32_t i = w * 32 + (uint32_t)(__ffs((int)bits) - 1);
                        bits &= bits - 1;
                        if (!(max_flags[i >> 5] >> (i & 31) & 1u)) continue;
                        const uint32_t info = rowinfo[i], v = info >> 6;
                        bool is_max = true;
                        for (uint32_t t = a.M.nbr_off[i]; t < a.M.nbr_off[i + 1]; ++t) {
                            const uint32_t j = a.M.nbr_idx[t];
                            if (v < (rowinfo[j] >> 6))
                                is_max = false;
                            else
                                max_flags[j >> 5] &= ~(1u << (j & 31));
                        }
                        if (is_max) {
                            max_flags[i >> 5] |= 1u << (i & 31);
                            const uint32_t slot = atomicAdd(a.out_count, 1u);
                            if (slot < a.out_cap) a.out[slot] = PpfMaximum{r, i, info & 63u, v};
                        } else {
                            max_flags[i >> 5] &= ~(1u << (i & 31));
                        }
                    }
                }
            }
        }
        __syncthreads();
        ppf_scene_pass<true>(a, p0, n0, frame, flags, acc, lane, wave, waves, &increments);
    }
    increments = wave_sum(increments);
    if (lane == 0 && increments) atomicAdd(&a.counters[1], increments);
    if (tid == 0 && visited) atomicAdd(&a.counters[0], visited);
}

uint32_t blocks_of(unsigned long long n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

}  // namespace

void launch_ppf_pair_keys(const PpfModelView& M, uint32_t* keys, hipStream_t st) {
    const unsigned long long pairs = (unsigned long long)M.n * M.n_e;
    const uint32_t blocks = (uint32_t)std::min<unsigned long long>((pairs + 255) / 256, 1u << 16);
    ppf_pair_keys_k<<<blocks, 256, 0, st>>>(M, keys);
}

void launch_ppf_cell_offsets(const uint32_t* sorted_keys, uint32_t pairs, uint32_t table_size, uint32_t* cell_off, hipStream_t st) {
    ppf_cell_offsets_k<<<blocks_of(pairs, 256), 256, 0, st>>>(sorted_keys, pairs, table_size, cell_off);
}

void launch_ppf_entries(const uint32_t* sorted_keys, const uint32_t* sorted_pairs, uint32_t n_entries, uint32_t n_e, uint32_t table_size,
                        uint32_t* entries, hipStream_t st) {
    if (n_entries == 0) return;
    ppf_entries_k<<<blocks_of(n_entries, 256), 256, 0, st>>>(sorted_keys, sorted_pairs, n_entries, n_e, table_size, entries);
}

void launch_ppf_nbr_count(const double* pts, uint32_t n, double r2, uint32_t* counts, hipStream_t st) {
    ppf_nbr_count_k<<<blocks_of(n, 64), 64, 0, st>>>(pts, n, r2, counts);
}

void launch_ppf_nbr_fill(const double* pts, uint32_t n, double r2, const uint32_t* offsets, uint32_t* idx, hipStream_t st) {
    ppf_nbr_fill_k<<<blocks_of(n, 64), 64, 0, st>>>(pts, n, r2, offsets, idx);
}

hipError_t launch_ppf_vote(const PpfVoteArgs& a, uint32_t groups, bool lds, hipStream_t st) {
    const size_t bytes = 4 * (2 * ppf_bitmap_words(a.M.n) + (lds ? (size_t)a.acc_words : 0));
    if (lds) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ppf_vote_k<true>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
        ppf_vote_k<true><<<groups, kPpfVoteThreads, bytes, st>>>(a);
    } else {
        ppf_vote_k<false><<<groups, kPpfVoteThreads, bytes, st>>>(a);
    }
    return hipGetLastError();
}

}  // namespace m3d
