// m3d_ppf.hpp -- launchers of the PPF table and vote kernels (m3d_ppf.hip), called by m3d_ppf.cpp.  The contract is in
// include/misc3d_amd.h ("PPF voting"), the arithmetic in m3d_ppf_fp.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "m3d_ppf_fp.hpp"

namespace m3d {

constexpr uint32_t kPpfMaxPoints = 65535;                 // a model index is 16 bits of a table entry
constexpr uint32_t kPpfMaxTableSize = 1u << 24;           // a pair's sort key: cell in bits 0-23, quant_alpha above
constexpr uint32_t kPpfKeyCellMask = kPpfMaxTableSize - 1;
constexpr int kPpfVoteThreads = 512;                      // one workgroup per reference point
constexpr size_t kPpfLdsAccBytes = 140 * 1024;            // accumulator bytes a workgroup may hold in LDS (one workgroup per CU;
                                                          // the two row bitmaps, at most 16 KiB, lie beside it)

// n x alpha_num 16-bit counters, two per 32-bit word
inline size_t ppf_acc_words(uint32_t n, int alpha_num) { return ((size_t)n * (size_t)alpha_num + 1) / 2; }
// the accumulator path: a function of (n, alpha_num) only
inline bool ppf_acc_in_lds(uint32_t n, int alpha_num) { return ppf_acc_words(n, alpha_num) * 4 <= kPpfLdsAccBytes; }
inline size_t ppf_bitmap_words(uint32_t n) { return ((size_t)n + 31) / 32; }

// The resident model as the kernels read it (T.dist_edge2 points at device memory).  The table pairs the reference set
// (pts, nrm, n) with the referred set (epts, enrm, n_e): the model's edge points in EdgePoints mode; in SampledPoints mode
// the referred set IS the reference set (same pointers, n_e == n, same_set) and the pairs i == j are left out.
struct PpfModelView {
    PpfTables T;
    uint32_t n, table_size;
    const double *pts, *nrm, *frames;   // n x 3 centred points, n x 3 normals, n x 8 (rows 1 and 2 of tmg)
    const double *epts, *enrm;          // n_e x 3 each: the referred set, centred by the same centroid
    uint32_t n_e;
    bool same_set;
    const uint32_t* cell_off;           // table_size + 1
    const uint32_t* entries;            // i | quant_alpha << 16, within a cell ascending (i, j)
    const uint32_t *nbr_off, *nbr_idx;  // n + 1 / the neighbour lists, ascending
};

struct PpfMaximum {   // one local maximum
    uint32_t ref_pos, model_index, alpha_index, votes;
};

struct PpfVoteArgs {
    PpfModelView M;
    const double *rpts, *rnrm;   // the cloud the reference points are read from, indexed by ref[]
    const double *spts, *snrm;   // m x 3 each: the cloud that is scanned for neighbours (SampledPoints: the same cloud;
                                 // EdgePoints: the n_ref reference points gathered, ref[] = 0 .. n_ref - 1, and the scene's edges)
    uint32_t m, n_ref;
    const uint32_t* ref;         // n_ref indices into rpts / rnrm
    const double* sframes;       // n_ref x 8 (rows 1 and 2 of tsg)
    double r2, dist_thresh, cos_thresh;
    uint32_t gate;               // size_t(n_e * 0.2): the vote runs for n_searched > gate, maxima need max_votes >= gate
    uint32_t acc_words;
    unsigned long long* flags;   // groups x table_size, zero on entry and on exit
    uint32_t* acc;               // groups x acc_words (device-memory path), else null
    uint32_t* rowinfo;           // groups x n: votes << 6 | alpha index of every row's best window
    PpfMaximum* out;
    uint32_t out_cap;
    uint32_t* out_count;                 // maxima found (may exceed out_cap: nothing is written past it)
    unsigned long long* counters;        // [0] neighbours visited, [1] increments
};

// keys[i n_e + j] = cell | quant_alpha << 24 of the ordered pair (i, j), or table_size for a pair that is skipped
void launch_ppf_pair_keys(const PpfModelView& M, uint32_t* keys, hipStream_t st);
// sorted keys (low 24 bits ascending) -> cell_off[0 .. table_size]; cell_off[table_size] = the number of entries
void launch_ppf_cell_offsets(const uint32_t* sorted_keys, uint32_t pairs, uint32_t table_size, uint32_t* cell_off, hipStream_t st);
// entries[t], t < n_entries, from the first n_entries sorted (key, pair index) pairs; i = pair index / n_e
void launch_ppf_entries(const uint32_t* sorted_keys, const uint32_t* sorted_pairs, uint32_t n_entries, uint32_t n_e, uint32_t table_size,
                        uint32_t* entries, hipStream_t st);
// counts[i] = the points j (i included) with d2 < r2; ... and, offsets being their exclusive scan, the lists
void launch_ppf_nbr_count(const double* pts, uint32_t n, double r2, uint32_t* counts, hipStream_t st);
void launch_ppf_nbr_fill(const double* pts, uint32_t n, double r2, const uint32_t* offsets, uint32_t* idx, hipStream_t st);
// the vote: `groups` workgroups, each takes the reference positions group, group + groups, ...
hipError_t launch_ppf_vote(const PpfVoteArgs& a, uint32_t groups, bool lds, hipStream_t st);

}  // namespace m3d
