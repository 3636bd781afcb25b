// test_raycast_fp.cpp -- host check of misc3d_amd/csrc/m3d_raycast_fp.hpp, the arithmetic the ray casting kernels run: no GPU,
// no library.  Built and run by tests/test_raycast.py together with tests/cpp/raycast_ref.c.
//   1. the monotonicity the culling rests on: for boxes A inside B and any ray from the origin, slab(B) contains slab(A),
//      lower(B) <= lower(A), and a box that may hold a hit implies the same of every box around it; the consequence the
//      traversal uses: a triangle that rule 3 accepts at t is never culled through a box around it at best_t == t;
//   2. rule 3 (ray_triangle) against the plain-C restatement, pair by pair, bit for bit.
// Prints one line per group and returns the number of failures.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "../../misc3d_amd/csrc/m3d_raycast_fp.hpp"

extern "C" int raycast_ref_pair(const float* d, const float* v0, const float* v1, const float* v2, float* t);

using namespace m3d;

static std::mt19937_64 rng(20240607);
static double uni(double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); }
static float step(float x, int ulps) {   // x moved by `ulps` representable numbers
    for (int k = 0; k < (ulps < 0 ? -ulps : ulps); ++k) x = std::nextafter(x, ulps < 0 ? -INFINITY : INFINITY);
    return x;
}

static float pick_coord(int kind) {
    switch (kind) {
        case 0: return (float)uni(-3, 3);
        case 1: return (float)uni(-1e-3, 1e-3);
        case 2: return (float)(uni(-1, 1) * std::pow(10.0, uni(-30, 30)));
        case 3: return 0.0f;
        case 4: return (float)uni(0.5, 5);
        default: return (float)uni(-5, -0.5);
    }
}

static float pick_dir(int kind) {
    switch (kind) {
        case 0: return (float)uni(-1, 1);
        case 1: return 0.0f;
        case 2: return -0.0f;
        case 3: return (float)(uni(-1, 1) * std::pow(10.0, uni(-44, -30)));   // subnormal and near: 1 / d overflows
        case 4: return (float)(uni(-1, 1) * std::pow(10.0, uni(20, 37)));
        default: return (float)uni(-1e-3, 1e-3);
    }
}

// A (lo, hi) and B around it; shape: what kind of boxes
static void make_boxes(int shape, float alo[3], float ahi[3], float blo[3], float bhi[3]) {
    for (int c = 0; c < 3; ++c) {
        int kind = 0;
        if (shape == 1) kind = (int)(rng() % 6);               // adversarial magnitudes and zeros
        if (shape == 2) kind = rng() % 2 ? 3 : 0;              // flat boxes, faces on 0
        if (shape == 4) kind = c == 2 ? 5 : 0;                 // behind the camera
        float x = pick_coord(kind), y = shape == 2 && rng() % 2 ? x : pick_coord(kind);
        if (shape == 3) {                                      // the origin inside (or on a face)
            x = -(float)std::fabs(pick_coord(rng() % 4));
            y = (float)std::fabs(pick_coord(rng() % 4));
        }
        alo[c] = x < y ? x : y;
        ahi[c] = x < y ? y : x;
        // B: equal, a few ulps wider, or much wider
        const int m = (int)(rng() % 4);
        blo[c] = m == 0 ? alo[c] : m == 1 ? step(alo[c], -(int)(rng() % 3)) : alo[c] - (float)std::fabs(pick_coord(rng() % 3));
        const int k = (int)(rng() % 4);
        bhi[c] = k == 0 ? ahi[c] : k == 1 ? step(ahi[c], (int)(rng() % 3)) : ahi[c] + (float)std::fabs(pick_coord(rng() % 3));
    }
}

static int check_monotone(const char* name, int shape, int n) {
    int bad = 0;
    for (int it = 0; it < n; ++it) {
        float alo[3], ahi[3], blo[3], bhi[3], d[3];
        make_boxes(shape, alo, ahi, blo, bhi);
        for (int c = 0; c < 3; ++c) d[c] = pick_dir(shape == 0 ? 0 : (int)(rng() % 6));
        if (rng() % 2) d[2] = 1.0f;   // the camera's rays
        float aa, ab, ba, bb;
        const bool aok = ray_slab(d, alo, ahi, &aa, &ab), bok = ray_slab(d, blo, bhi, &ba, &bb);
        bool fail = false;
        if (aok && !bok) fail = true;
        if (!(ba <= aa) || !(bb >= ab)) fail = true;   // (a and b are never NaN: they start as numbers and only take numbers)
        const float la = ray_lower(aa, ab), lb = ray_lower(ba, bb);
        if (la == la && lb == lb && !(lb <= la)) fail = true;
        const float best = rng() % 3 == 0 ? INFINITY : (float)uni(0, 6);
        float l0, l1;
        if (ray_box_may_hit(d, alo, ahi, best, &l0) && !ray_box_may_hit(d, blo, bhi, best, &l1)) fail = true;
        if (fail && bad++ < 5)
            std::printf("  monotonicity broken: d = (%a, %a, %a) A = [%a %a %a, %a %a %a] B = [%a %a %a, %a %a %a]\n", d[0], d[1], d[2],
                        alo[0], alo[1], alo[2], ahi[0], ahi[1], ahi[2], blo[0], blo[1], blo[2], bhi[0], bhi[1], bhi[2]);
    }
    std::printf("%s: %d boxes, %d failures\n", name, n, bad);
    return bad;
}

static void random_triangle(int kind, float v[3][3], float d[3]) {
    const double z = kind == 3 ? uni(-3, 3) : uni(0.5, 4);
    for (int k = 0; k < 3; ++k) {
        v[k][0] = (float)uni(-2, 2);
        v[k][1] = (float)uni(-2, 2);
        v[k][2] = (float)(z + uni(-0.5, 0.5));
    }
    if (kind == 1)   // a sliver
        for (int c = 0; c < 3; ++c) v[2][c] = v[0][c] + (v[1][c] - v[0][c]) * 0.5f + (float)uni(-1e-6, 1e-6);
    if (kind == 2)   // zero area
        for (int c = 0; c < 3; ++c) v[2][c] = v[rng() % 2][c];
    if (kind == 4)   // huge and tiny coordinates: products overflow and underflow
        for (int k = 0; k < 3; ++k)
            for (int c = 0; c < 3; ++c) v[k][c] *= rng() % 2 ? 1e30f : 1e-30f;
    // a ray through a point of the triangle (or near an edge or a vertex of it), or any ray
    double w0 = uni(0, 1), w1 = uni(0, 1 - w0);
    const int where = (int)(rng() % 4);
    if (where == 1) w1 = 1 - w0;   // on an edge
    if (where == 2) w0 = 1, w1 = 0;   // on a vertex
    const double w2 = 1 - w0 - w1;
    double p[3];
    for (int c = 0; c < 3; ++c) p[c] = w0 * v[0][c] + w1 * v[1][c] + w2 * v[2][c];
    if (where == 3 || p[2] == 0) {
        d[0] = (float)uni(-1, 1);
        d[1] = (float)uni(-1, 1);
    } else {
        d[0] = (float)(p[0] / p[2]);
        d[1] = (float)(p[1] / p[2]);
    }
    if (rng() % 16 == 0) d[rng() % 2] = 0.0f;
    d[2] = 1.0f;
}

static int check_pairs(int n) {
    int bad = 0;
    long hits = 0, culled = 0;
    for (int it = 0; it < n; ++it) {
        float v[3][3], d[3];
        random_triangle(it % 5, v, d);
        float t0 = 0.0f, t1 = 0.0f;
        const bool ours = ray_triangle(d, v[0], v[1], v[2], &t0);
        const int ref = raycast_ref_pair(d, v[0], v[1], v[2], &t1);
        hits += ours;
        culled += ref == 1;
        bool fail = ours != (ref == 3);
        if (ours && std::memcmp(&t0, &t1, 4) != 0) fail = true;
        // what the traversal relies on: no box around an accepted triangle is culled at best_t == t
        if (ours) {
            float lo[3], hi[3], low;
            for (int c = 0; c < 3; ++c) {
                lo[c] = rc_min(rc_min(v[0][c], v[1][c]), v[2][c]) - (float)(rng() % 3) * (float)std::fabs(uni(0, 1));
                hi[c] = rc_max(rc_max(v[0][c], v[1][c]), v[2][c]) + (float)(rng() % 3) * (float)std::fabs(uni(0, 1));
            }
            if (!ray_box_may_hit(d, lo, hi, t0, &low)) fail = true;
        }
        if (fail && bad++ < 5) std::printf("  pair %d: ours %d t %a, reference %d t %a\n", it, (int)ours, t0, ref, t1);
    }
    std::printf("pairs: %d tested, %ld hits, %ld Moeller-Trumbore hits the clause rejects, %d failures\n", n, hits, culled, bad);
    if (hits < n / 20) {
        std::printf("  too few hits for the comparison to mean anything\n");
        ++bad;
    }
    return bad;
}

int main() {
    int bad = 0;
    bad += check_monotone("random", 0, 400000);
    bad += check_monotone("adversarial", 1, 400000);
    bad += check_monotone("flat", 2, 200000);
    bad += check_monotone("origin inside", 3, 200000);
    bad += check_monotone("behind the camera", 4, 200000);
    bad += check_pairs(1000000);
    // the normal of rule 4: zero and overflowing squared lengths give (0, 0, 0)
    {
        const float a[3] = {0, 0, 1}, b[3] = {1, 0, 1}, c[3] = {0, 1, 1}, big[3] = {1e30f, 0, 1}, big2[3] = {0, 1e30f, 1};
        float n[3];
        triangle_normal(a, b, c, n);
        if (!(n[0] == 0 && n[1] == 0 && n[2] == 1)) ++bad;
        triangle_normal(a, b, b, n);
        if (!(n[0] == 0 && n[1] == 0 && n[2] == 0)) ++bad;
        triangle_normal(a, big, big2, n);
        if (!(n[0] == 0 && n[1] == 0 && n[2] == 0)) ++bad;
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
