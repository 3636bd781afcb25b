// m3d_raycast_fp.hpp -- the arithmetic of the ray casting contract (include/misc3d_amd.h, m3d_raycast_pinhole, rules 1-4):
// the ONE place the pixel's ray, the vertex transform, the slab interval and the (ray, triangle) test exist.  Shared by the
// kernels (m3d_raycast.hip) and a host check (tests/cpp/test_raycast_fp.cpp); no dependency on M3D_FP_ORDER (no sum here is
// left to an association: every one is written out).
//
// Number formats: rule 1 and rule 2 are fp64 rounded ONCE to fp32; everything after is fp32 with every operation rounded
// separately (build with -ffp-contract=off), divisions and square roots correctly rounded and subnormals kept -- hipcc's
// defaults for gfx950 (-fhip-fp32-correctly-rounded-divide-sqrt, no denormal flushing) and every x86-64 compiler's.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define M3D_RC_HD __host__ __device__ __forceinline__
#else
#define M3D_RC_HD inline
#endif

namespace m3d {

constexpr uint32_t kRayInvalidId = 0xFFFFFFFFu;   // Open3D's RaycastingScene::INVALID_ID
constexpr float kRayLowerSlack = 1.52587890625e-05f;   // 2^-16 (rule 3: lower = a - 2^-16 b)

struct RayHit {   // the running best of rule 4
    float t;
    uint32_t geom, prim;
};

// rule 1: direction of pixel (x, y); computed in fp64, rounded once
M3D_RC_HD void ray_direction(uint32_t x, uint32_t y, double fx, double fy, double cx, double cy, float d[3]) {
    d[0] = (float)((((double)x + 0.5) - cx) / fx);
    d[1] = (float)((((double)y + 0.5) - cy) / fy);
    d[2] = 1.0f;
}

// rule 2: p' = R p + t of the row-major 4 x 4 pose T (its last row is not read), ((T0 x + T1 y) + T2 z) + T3 per row in
// fp64, rounded once
M3D_RC_HD void transform_vertex(const double* T, double x, double y, double z, float out[3]) {
    for (int r = 0; r < 3; ++r) out[r] = (float)(((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3]);
}

M3D_RC_HD float rc_min(float a, float b) { return b < a ? b : a; }
M3D_RC_HD float rc_max(float a, float b) { return b > a ? b : a; }

// slab(ray, box) of rule 3 for a ray from the origin: *a = max(0, near values), *b = min(far values) over the axes with
// d != 0; an axis with d == 0 fails the box unless lo <= 0 <= hi.  A product that is NaN (0 * inf: 1 / d overflowed)
// constrains nothing: the comparisons below are false for it.  Boxes are finite (the transform refuses anything else), so
// no other NaN arises.  Returns false when the box fails outright; the caller still tests *a <= *b.
M3D_RC_HD bool ray_slab(const float d[3], const float lo[3], const float hi[3], float* a, float* b) {
    float ta = 0.0f, tb = INFINITY;
    bool ok = true;
    for (int c = 0; c < 3; ++c) {
        if (d[c] != 0.0f) {
            const float inv = 1.0f / d[c];
            const float t0 = lo[c] * inv, t1 = hi[c] * inv;
            const float tn = d[c] > 0.0f ? t0 : t1, tf = d[c] > 0.0f ? t1 : t0;
            if (tn > ta) ta = tn;
            if (tf < tb) tb = tf;
        } else if (!(lo[c] <= 0.0f && 0.0f <= hi[c])) {
            ok = false;
        }
    }
    *a = ta;
    *b = tb;
    return ok;
}

// lower(box): no hit inside the box is accepted below it
M3D_RC_HD float ray_lower(float a, float b) { return a - kRayLowerSlack * b; }

// What a traversal asks of a node's box: may it hold an accepted hit that beats (or ties) best_t?  Monotone in the box:
// false for a box implies false for every box inside it (DESIGN.md "Ray casting").  *lower is for ordering only.
M3D_RC_HD bool ray_box_may_hit(const float d[3], const float lo[3], const float hi[3], float best_t, float* lower) {
    float a, b;
    const bool ok = ray_slab(d, lo, hi, &a, &b);
    const float l = ray_lower(a, b);
    *lower = l;
    return ok && a <= b && !(l > best_t);
}

M3D_RC_HD void rc_cross(const float a[3], const float b[3], float out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}
M3D_RC_HD float rc_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// rule 3: the (ray, triangle) test.  True: *t is the hit's parameter.
M3D_RC_HD bool ray_triangle(const float d[3], const float v0[3], const float v1[3], const float v2[3], float* t) {
    float e1[3], e2[3], s[3], p[3], q[3], lo[3], hi[3];
    for (int c = 0; c < 3; ++c) {
        e1[c] = v1[c] - v0[c];
        e2[c] = v2[c] - v0[c];
        s[c] = -v0[c];
        lo[c] = rc_min(rc_min(v0[c], v1[c]), v2[c]);
        hi[c] = rc_max(rc_max(v0[c], v1[c]), v2[c]);
    }
    rc_cross(d, e2, p);
    const float det = rc_dot(e1, p);
    const float u = rc_dot(s, p) / det;
    rc_cross(s, e1, q);
    const float v = rc_dot(d, q) / det;
    const float tt = rc_dot(e2, q) / det;
    if (!(det != 0.0f && u >= 0.0f && v >= 0.0f && u + v <= 1.0f && tt > 0.0f && tt < INFINITY)) return false;
    float a, b;
    if (!ray_slab(d, lo, hi, &a, &b) || !(a <= b) || !(tt >= ray_lower(a, b))) return false;
    *t = tt;
    return true;
}

// rule 4: does (t, geom, prim) beat the running best?
M3D_RC_HD bool ray_hit_better(float t, uint32_t geom, uint32_t prim, const RayHit& best) {
    if (t != best.t) return t < best.t;
    if (geom != best.geom) return geom < best.geom;
    return prim < best.prim;
}

// rule 4: the primitive normal, normalize((v1 - v0) x (v2 - v0)); (0, 0, 0) when its squared length is 0 or not finite
M3D_RC_HD void triangle_normal(const float v0[3], const float v1[3], const float v2[3], float n[3]) {
    float e1[3], e2[3], c[3];
    for (int k = 0; k < 3; ++k) {
        e1[k] = v1[k] - v0[k];
        e2[k] = v2[k] - v0[k];
    }
    rc_cross(e1, e2, c);
    const float len2 = rc_dot(c, c);
    if (!(len2 > 0.0f && len2 < INFINITY)) {
        n[0] = n[1] = n[2] = 0.0f;
        return;
    }
    const float len = sqrtf(len2);
    for (int k = 0; k < 3; ++k) n[k] = c[k] / len;
}

}  // namespace m3d
