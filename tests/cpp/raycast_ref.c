/* raycast_ref.c -- the ray casting contract of include/misc3d_amd.h (m3d_raycast_pinhole, rules 1-4) restated as a brute force
 * over every (ray, triangle) pair: no hierarchy, no culling, nothing shared with the library's sources.  Built by
 * tests/raycast_ref_util.py with gcc -O2 -ffp-contract=off (every operation rounded separately; x86-64 evaluates float in
 * float); with -fopenmp the rows of the image are shared among threads (the benchmark's CPU baseline).
 *
 * Besides the four maps it counts what the culling clause of rule 3 does: the pairs that pass the five Moeller-Trumbore
 * comparisons, those of them the clause rejects, and the pixels whose answer the clause changes. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define INVALID_ID 0xFFFFFFFFu

typedef struct { /* what every pair reads: 36 bytes a triangle, so that a scene stays in the cache while the pixels go by */
    float e1[3], e2[3], s[3]; /* v1 - v0, v2 - v0, -v0 */
} edges_t;
typedef struct {
    float v[3][3];
    float lo[3], hi[3];
    uint32_t geom, prim;
} tri_t;

static float min3(float a, float b, float c) {
    float m = a;
    if (b < m) m = b;
    if (c < m) m = c;
    return m;
}
static float max3(float a, float b, float c) {
    float m = a;
    if (b > m) m = b;
    if (c > m) m = c;
    return m;
}

static void cross(const float *a, const float *b, float *o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
static float dot(const float *a, const float *b) {
    float s = a[0] * b[0] + a[1] * b[1];
    return s + a[2] * b[2];
}

/* the comparisons of rule 3 in the rule's order, each value computed when its turn comes (a comparison that fails ends the
 * test; what the later values would have been changes nothing); 1 = they all pass, *t set */
static int moller_trumbore(const float *d, const edges_t *tr, float *t) {
    float p[3], q[3], det, u, v, tt;
    cross(d, tr->e2, p);
    det = dot(tr->e1, p);
    if (!(det != 0.0f)) return 0;
    u = dot(tr->s, p) / det;
    if (!(u >= 0.0f)) return 0;
    cross(tr->s, tr->e1, q);
    v = dot(d, q) / det;
    if (!(v >= 0.0f)) return 0;
    if (!(u + v <= 1.0f)) return 0;
    tt = dot(tr->e2, q) / det;
    if (!(tt > 0.0f && tt < INFINITY)) return 0;
    *t = tt;
    return 1;
}

/* the clause: 1 = the slab of the triangle's box is non-empty and t >= a - 2^-16 b */
static int clause(const float *d, const tri_t *tr, float t) {
    float a = 0.0f, b = INFINITY;
    int c;
    for (c = 0; c < 3; ++c) {
        if (d[c] != 0.0f) {
            const float inv = 1.0f / d[c];
            const float x = tr->lo[c] * inv, y = tr->hi[c] * inv;
            const float tn = d[c] > 0.0f ? x : y, tf = d[c] > 0.0f ? y : x;
            if (tn > a) a = tn; /* a NaN product compares false: no constraint */
            if (tf < b) b = tf;
        } else if (!(tr->lo[c] <= 0.0f && 0.0f <= tr->hi[c])) {
            return 0;
        }
    }
    if (!(a <= b)) return 0;
    return t >= a - 0x1p-16f * b;
}

static void finish(tri_t *tr, edges_t *ed) {
    int c;
    for (c = 0; c < 3; ++c) {
        ed->e1[c] = tr->v[1][c] - tr->v[0][c];
        ed->e2[c] = tr->v[2][c] - tr->v[0][c];
        ed->s[c] = -tr->v[0][c];
        tr->lo[c] = min3(tr->v[0][c], tr->v[1][c], tr->v[2][c]);
        tr->hi[c] = max3(tr->v[0][c], tr->v[1][c], tr->v[2][c]);
    }
}

static int better(float t, uint32_t g, uint32_t p, float bt, uint32_t bg, uint32_t bp) {
    if (t < bt) return 1;
    if (t > bt) return 0;
    if (g != bg) return g < bg;
    return p < bp;
}

/* verts: all meshes' vertices one after the other, vert_off[g] .. vert_off[g + 1] those of mesh g; tris likewise, indices
 * local to the mesh; poses: n_mesh row-major 4 x 4.  counts[0] = Moeller-Trumbore hits, [1] = those the clause rejects,
 * [2] = pixels the clause changes.  Returns 0, or 3 when a transformed vertex is not finite in fp32 (counts[0] = its
 * global index). */
int raycast_ref(const double *verts, const uint64_t *vert_off, const int32_t *tris, const uint64_t *tri_off, uint64_t n_mesh,
                const double *poses, int W, int H, double fx, double fy, double cx, double cy, float *t_hit, uint32_t *geom,
                uint32_t *prim, float *normals, uint64_t *counts) {
    const uint64_t nv = vert_off[n_mesh], nt = tri_off[n_mesh];
    float *v32 = (float *)malloc(sizeof(float) * 3 * (nv ? nv : 1));
    tri_t *tr = (tri_t *)malloc(sizeof(tri_t) * (nt ? nt : 1));
    edges_t *ed = (edges_t *)malloc(sizeof(edges_t) * (nt ? nt : 1));
    uint64_t g, i, n_mt = 0, n_rej = 0, n_changed = 0;
    int y, c;
    counts[0] = counts[1] = counts[2] = 0;
    for (g = 0; g < n_mesh; ++g) {
        const double *T = poses + 16 * g;
        for (i = vert_off[g]; i < vert_off[g + 1]; ++i) {
            const double px = verts[3 * i], py = verts[3 * i + 1], pz = verts[3 * i + 2];
            for (c = 0; c < 3; ++c) {
                double s = T[4 * c] * px + T[4 * c + 1] * py;
                s = s + T[4 * c + 2] * pz;
                s = s + T[4 * c + 3];
                v32[3 * i + c] = (float)s;
                if (!isfinite(v32[3 * i + c])) {
                    counts[0] = i;
                    free(v32);
                    free(tr);
                    free(ed);
                    return 3;
                }
            }
        }
        for (i = tri_off[g]; i < tri_off[g + 1]; ++i) {
            int k;
            for (k = 0; k < 3; ++k)
                for (c = 0; c < 3; ++c) tr[i].v[k][c] = v32[3 * (vert_off[g] + (uint64_t)tris[3 * i + k]) + c];
            finish(&tr[i], &ed[i]);
            tr[i].geom = (uint32_t)g;
            tr[i].prim = (uint32_t)(i - tri_off[g]);
        }
    }
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : n_mt, n_rej, n_changed)
    for (y = 0; y < H; ++y) {
        int x;
        for (x = 0; x < W; ++x) {
            const size_t pix = (size_t)y * (size_t)W + (size_t)x;
            float d[3], bt = INFINITY, ft = INFINITY;
            uint32_t bg = INVALID_ID, bp = INVALID_ID, fg = INVALID_ID, fp = INVALID_ID;
            uint64_t k, bi = 0;
            d[0] = (float)((((double)x + 0.5) - cx) / fx);
            d[1] = (float)((((double)y + 0.5) - cy) / fy);
            d[2] = 1.0f;
            for (k = 0; k < nt; ++k) {
                float t;
                if (!moller_trumbore(d, &ed[k], &t)) continue;
                ++n_mt;
                if (better(t, tr[k].geom, tr[k].prim, ft, fg, fp)) { /* without the clause */
                    ft = t;
                    fg = tr[k].geom;
                    fp = tr[k].prim;
                }
                if (!clause(d, &tr[k], t)) {
                    ++n_rej;
                    continue;
                }
                if (better(t, tr[k].geom, tr[k].prim, bt, bg, bp)) {
                    bt = t;
                    bg = tr[k].geom;
                    bp = tr[k].prim;
                    bi = k;
                }
            }
            if (!(ft == bt && fg == bg && fp == bp)) ++n_changed;
            if (t_hit) t_hit[pix] = bt;
            if (geom) geom[pix] = bg;
            if (prim) prim[pix] = bp;
            if (normals) {
                float n[3] = {0.0f, 0.0f, 0.0f};
                if (bg != INVALID_ID) {
                    float e1[3], e2[3], cr[3], l2;
                    for (c = 0; c < 3; ++c) {
                        e1[c] = tr[bi].v[1][c] - tr[bi].v[0][c];
                        e2[c] = tr[bi].v[2][c] - tr[bi].v[0][c];
                    }
                    cross(e1, e2, cr);
                    l2 = dot(cr, cr);
                    if (l2 > 0.0f && l2 < INFINITY) {
                        const float l = sqrtf(l2);
                        for (c = 0; c < 3; ++c) n[c] = cr[c] / l;
                    }
                }
                for (c = 0; c < 3; ++c) normals[3 * pix + c] = n[c];
            }
        }
    }
    counts[0] = n_mt;
    counts[1] = n_rej;
    counts[2] = n_changed;
    free(v32);
    free(tr);
    free(ed);
    return 0;
}

/* one pair, for tests/cpp/test_raycast_fp.cpp: bit 0 = the Moeller-Trumbore comparisons pass, bit 1 = the clause passes too */
int raycast_ref_pair(const float *d, const float *v0, const float *v1, const float *v2, float *t) {
    tri_t tr;
    edges_t ed;
    int c;
    float tt = 0.0f;
    for (c = 0; c < 3; ++c) {
        tr.v[0][c] = v0[c];
        tr.v[1][c] = v1[c];
        tr.v[2][c] = v2[c];
    }
    finish(&tr, &ed);
    if (!moller_trumbore(d, &ed, &tt)) return 0;
    *t = tt;
    return clause(d, &tr, tt) ? 3 : 1;
}
