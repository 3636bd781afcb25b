// m3d_orient.hpp -- launchers of the normal orientation's kernels (m3d_orient.hip), called by m3d_orient.cpp: the minimum
// spanning forest of the radius graph by Boruvka rounds over the cell-sorted grid (include/misc3d_amd.h, "PPF model
// preprocessing", rules O1 - O3).  Vertices are GRID SLOTS t (the points in cell order); orig[t] is the point's index.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "m3d_reg_kernels.hpp"

namespace m3d {

constexpr uint32_t kOrientNone = 0xFFFFFFFFu;
constexpr unsigned long long kOrientNoKey = ~0ull;

// what the rounds keep per slot (n entries each unless stated); every word is written by launch_orient_init
struct OrientState {
    uint32_t* parent;             // union-find over slots (m3d_union_find.hpp)
    uint32_t* comp;               // parent[] flattened at the end of the last round: the slot's component label
    uint32_t* slot_of;            // slot_of[orig[t]] = t
    uint32_t* best_u;             // the other end of the slot's least edge that leaves its component, kOrientNone: none
    double* best_d2;              // ... and its d2
    uint32_t* dead;               // 1: the slot's whole neighbourhood carried its label once -- it never has such an edge again
    unsigned long long* min_d2;   // per label: the bits of the least d2 among its slots' edges (pass one), kOrientNoKey: none
    unsigned long long* min_e;    // per label: lo << 32 | hi of its least edge (pass two), in point indices
    uint32_t* edges;              // 2 (n - 1): the tree edges (lo, hi) in point indices, in no particular order
    uint32_t* n_edges;            // 1
};

void launch_orient_init(const OrientState& s, const uint32_t* orig, uint32_t n, hipStream_t st);
// pass one: every live slot's least edge under (d2, lo, hi) to a slot of another label, and the label's least d2
void launch_orient_scan(const GridDesc& g, const uint32_t* cell_start, const double* qx, const double* qy, const double* qz,
                        const uint32_t* orig, const OrientState& s, uint32_t n, hipStream_t st);
// pass two: among the slots whose own least edge has their label's least d2, the least (lo, hi)
void launch_orient_pick(const uint32_t* orig, const OrientState& s, uint32_t n, hipStream_t st);
// every label's edge hooked and appended to the edge list once
void launch_orient_hook(const OrientState& s, uint32_t n, hipStream_t st);
// comp[] = the roots after the hooks; min_d2 / min_e reset for the next round
void launch_orient_flatten(const OrientState& s, uint32_t n, hipStream_t st);

}  // namespace m3d
