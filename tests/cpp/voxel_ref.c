/* voxel_ref.c -- the voxel down-sampling contract restated in plain C: the checker of m3d_voxel_down_sample.
 *
 * [RECALL] Open3D 0.15.1 PointCloud::VoxelDownSample / AccumulatedPoint, written from the contract in
 * include/misc3d_amd.h (rules 1-7), on purpose without any code of the library: one thread, one hash map, the points
 * visited in ascending index.  Build with -ffp-contract=off.
 *
 *   vmin = min_bound - voxel_size * 0.5, vmax = max_bound + voxel_size * 0.5
 *   voxel_size * INT_MAX < max (vmax - vmin)  ->  "voxel_size is too small."
 *   voxel of p: (int)floor((p - vmin) / voxel_size) per coordinate
 *   per voxel: sums from +0.0, += in ascending point index; a normal with a NaN component is not added; / (double)count
 *   output order: ascending lowest member index (= the order in which a serial pass first sees the voxels)
 *
 * Returns 0, or 1 "[VoxelDownSample] voxel_size <= 0." (NaN too), 2 "[VoxelDownSample] voxel_size is too small.",
 * 3 a point with a non-finite coordinate (our deviation; *m = its index), 4 voxel_size = +inf or overflowing bounds. */
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    int32_t k[3];
    uint32_t id; /* output row + 1, 0 = empty */
} entry;

static uint64_t hash3(int32_t a, int32_t b, int32_t c) {
    uint64_t h = (uint64_t)(uint32_t)a * 0x9E3779B97F4A7C15ull;
    h ^= (uint64_t)(uint32_t)b * 0xC2B2AE3D27D4EB4Full + (h << 6) + (h >> 2);
    h ^= (uint64_t)(uint32_t)c * 0x165667B19E3779F9ull + (h << 6) + (h >> 2);
    h ^= h >> 29;
    return h;
}

int voxel_ref(const double *xyz, const double *normals, const double *colors, size_t n, double voxel_size, double *out_xyz,
              double *out_normals, double *out_colors, uint64_t *first_index, uint64_t *point_to_voxel, uint32_t *counts,
              size_t *m) {
    *m = 0;
    if (!(voxel_size > 0.0)) return 1;
    if (isinf(voxel_size)) return 4;
    if (n == 0) return 0;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c) {
            const double p = xyz[3 * i + c];
            if (!isfinite(p)) {
                *m = i;
                return 3;
            }
            if (p < lo[c]) lo[c] = p;
            if (p > hi[c]) hi[c] = p;
        }
    const double half = voxel_size * 0.5;
    double vmin[3], ext = -INFINITY;
    for (int c = 0; c < 3; ++c) {
        vmin[c] = lo[c] - half;
        const double vmax = hi[c] + half;
        const double e = vmax - vmin[c];
        if (e > ext) ext = e;
    }
    if (voxel_size * (double)INT_MAX < ext) return 2;
    if (!isfinite(ext)) return 4;
    size_t cap = 64;
    while (cap < 2 * n) cap *= 2;
    entry *tab = (entry *)calloc(cap, sizeof(entry));
    if (!tab) return -1;
    size_t rows = 0;
    for (size_t i = 0; i < n; ++i) {
        int32_t k[3];
        for (int c = 0; c < 3; ++c) {
            const double d = xyz[3 * i + c] - vmin[c];
            const double q = d / voxel_size;
            k[c] = (int)floor(q);
        }
        size_t s = (size_t)hash3(k[0], k[1], k[2]) & (cap - 1);
        while (tab[s].id && (tab[s].k[0] != k[0] || tab[s].k[1] != k[1] || tab[s].k[2] != k[2])) s = (s + 1) & (cap - 1);
        if (!tab[s].id) { /* first seen: a new output row, sums +0.0 */
            memcpy(tab[s].k, k, sizeof(k));
            tab[s].id = (uint32_t)(rows + 1);
            for (int c = 0; c < 3; ++c) {
                out_xyz[3 * rows + c] = 0.0;
                if (normals) out_normals[3 * rows + c] = 0.0;
                if (colors) out_colors[3 * rows + c] = 0.0;
            }
            counts[rows] = 0;
            if (first_index) first_index[rows] = i;
            ++rows;
        }
        const size_t j = tab[s].id - 1;
        for (int c = 0; c < 3; ++c) out_xyz[3 * j + c] += xyz[3 * i + c];
        if (normals) {
            const double *q = normals + 3 * i;
            if (!isnan(q[0]) && !isnan(q[1]) && !isnan(q[2]))
                for (int c = 0; c < 3; ++c) out_normals[3 * j + c] += q[c];
        }
        if (colors)
            for (int c = 0; c < 3; ++c) out_colors[3 * j + c] += colors[3 * i + c];
        counts[j] += 1;
        if (point_to_voxel) point_to_voxel[i] = j;
    }
    for (size_t j = 0; j < rows; ++j) {
        const double cnt = (double)counts[j];
        for (int c = 0; c < 3; ++c) {
            out_xyz[3 * j + c] = out_xyz[3 * j + c] / cnt;
            if (normals) out_normals[3 * j + c] = out_normals[3 * j + c] / cnt;
            if (colors) out_colors[3 * j + c] = out_colors[3 * j + c] / cnt;
        }
    }
    free(tab);
    *m = rows;
    return 0;
}
