// dsdf_eikonal.h -- per-voxel arithmetic of the redistancing kernels (dsdf_redistance.h): the frozen-band initialisation and the
// Godunov upwind update of |grad u| = 1.  Host/device inline functions like dsdf_math.h: tests/harness compiles the same
// statements for the CPU (hh_redistance) so that the suite can compare them with the fp64 oracle without a GPU.
#pragma once
#include "dsdf_math.h"

#define DSDF_RD_BIG 1e10f

namespace dsdf {

DSDF_HD float eik_sqrtf(float x) {            // v_sqrt_f32 (1 ulp) on the device
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sqrtf(x);
#else
    return sqrtf(x);
#endif
}
DSDF_HD float eik_med3f(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fmed3f(a, b, c);
#else
    return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c));
#endif
}

// Voxel i = (x, y, z) of phi: frozen at the sub-voxel distance D, 1/D^2 = sum_axes 1/d_a^2, when phi changes sign towards a
// 6-neighbour (or is exactly zero); DSDF_RD_BIG and free otherwise.  Returns the frozen flag.
DSDF_HD bool eikonal_init(const float *__restrict__ phi, size_t i, int x, int y, int z, int rx, int ry, int rz, float &u) {
    float p = phi[i];
    if (p == 0.f) { u = 0.f; return true; }
    const float h[3] = {1.f / rx, 1.f / ry, 1.f / rz};
    const int c[3] = {x, y, z}, dims[3] = {rx, ry, rz};
    const long strides[3] = {1, rx, (long)rx * ry};
    float inv2 = 0.f; bool any = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float d = DSDF_RD_BIG;
#pragma unroll
        for (int sgn = -1; sgn <= 1; sgn += 2) {
            int cn = c[a] + sgn;
            if (cn < 0 || cn >= dims[a]) continue;
            float q = phi[(long)i + sgn * strides[a]];
            if ((p > 0.f) != (q > 0.f)) d = fminf(d, h[a] * fabsf(p) / (fabsf(p) + fabsf(q)));
        }
        if (d < DSDF_RD_BIG) { inv2 += 1.f / (d * d); any = true; }
    }
    u = any ? 1.f / sqrtf(inv2) : DSDF_RD_BIG;
    return any;
}

// Godunov upwind update from the smallest neighbour value per axis, IN DIFFERENCES FROM THE SMALLEST OF THE THREE: with
// p = mid - lo, r = hi - lo the root t = u - lo solves sum_k w_k (t - d_k)^2 = 1 over the axes that take part (d = 0, p, r; w = 1/h^2).
// Every term of the discriminant is then of order h^2 like the discriminant itself.  (Written on the absolute values --
// s^2 - 3 (q - h^2) with s = a + b + c, q = a^2 + b^2 + c^2, and B^2 - 4 A C below -- it is a difference of numbers of order u^2:
// in fp32 that cost 0.26 voxel at 168^3 and 12 voxels on a 2 x 728 x 728 slab against the fp64 oracle, where this form stays
// below 0.001 and 0.01: profiles/redistance_precision.md.)
//
// Equal spacings h (cubic grids: every grid the optimiser uses): no per-axis weights, no divisions.
//   1 term: h;  2 terms: (p + sqrt(2 h^2 - p^2)) / 2;  3 terms: (s + sqrt(s^2 - 3 (p^2 + r^2 - h^2))) / 3, s = p + r
DSDF_HD float eikonal_update_iso(float a, float b, float c, float h) {
    const float lo = fminf(a, fminf(b, c)), hi = fmaxf(a, fmaxf(b, c));
    const float mid = eik_med3f(a, b, c);
    const float p = mid - lo, r = hi - lo;
    if (h <= p) return lo + h;
    float t = 0.5f * (p + eik_sqrtf(fmaxf(2.f * h * h - p * p, 0.f)));
    if (t <= r) return lo + t;
    const float s = p + r;
    t = (s + eik_sqrtf(fmaxf(s * s - 3.f * (p * p + r * r - h * h), 0.f))) * (1.f / 3.f);
    return lo + t;
}

DSDF_HD float eikonal_update(float a, float b, float c, float ha, float hb, float hc) {
    // sort (value, spacing) ascending by value
    if (a > b) { float t = a; a = b; b = t; t = ha; ha = hb; hb = t; }
    if (b > c) { float t = b; b = c; c = t; t = hb; hb = hc; hc = t; }
    if (a > b) { float t = a; a = b; b = t; t = ha; ha = hb; hb = t; }
    const float p = b - a, r = c - a;
    if (ha <= p) return a + ha;
    float w0 = 1.f / (ha * ha), w1 = 1.f / (hb * hb);
    {
        float A = w0 + w1, B = -2.f * (w1 * p), C = w1 * p * p - 1.f;
        float t = (-B + sqrtf(fmaxf(B * B - 4.f * A * C, 0.f))) / (2.f * A);
        if (t <= r) return a + t;
    }
    float w2 = 1.f / (hc * hc);
    float A = w0 + w1 + w2, B = -2.f * (w1 * p + w2 * r), C = w1 * p * p + w2 * r * r - 1.f;
    return a + (-B + sqrtf(fmaxf(B * B - 4.f * A * C, 0.f))) / (2.f * A);
}

}  // namespace dsdf
