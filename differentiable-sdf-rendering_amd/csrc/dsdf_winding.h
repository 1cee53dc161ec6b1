// dsdf_winding.h -- the generalized winding number of a triangle soup (Jacobson et al. 2013): w(x) = (1 / 4 pi) sum_t Omega_t(x), the
// signed solid angles of the triangles seen from x.  For a closed, outward-oriented mesh it is the integer number of times the surface
// wraps x (1 inside, 0 outside); for an open or dirty mesh it degrades smoothly and w > 0.5 is the inside test.  Brute force (every
// point against every triangle) and through the tree of dsdf_bvh.h with the far field of a subtree collapsed into one dipole (Barill et
// al. 2018, the first-order term).
//
// Two parts, like dsdf_bvh.h (which must be included first): host/device inline arithmetic that any C++ compiler builds -- the host-side
// tests run exactly these statements -- and, under __HIPCC__, the kernels and the C-ABI entry points (dsdf_kernels.hip includes this file
// after dsdf_mesh.h).
//
// MOMENTS.  The BVH buffer is ABI and stays as it is; the per-node moments live in a second caller-owned buffer of 16 L floats: one record
// of 8 floats per heap node, leaves included, the record of heap node i at 8 (i + 1) -- the two children of a node (2 i + 1, 2 i + 2) then
// sit at 16 (i + 1) and 16 (i + 1) + 8 and share one 64-byte line; the first 8 floats are int L (the tree the moments belong to: the walk
// refuses a buffer of another size with NaN instead of reading past it) and 7 x 0.  A record:
//   N.xyz   the area-weighted normal sum of the subtree, sum 1/2 e1 x e2
//   c.xyz   its area-weighted centroid, sum A_t (p0 + p1 + p2) / 3 / sum A_t (without area: the plain mean of what is there)
//   r       a radius such that every point of the subtree's triangles lies within r of c; -1: the subtree is EMPTY (skipped)
//   A       the total area sum |1/2 e1 x e2|, which the level pass needs to merge two centroids; A = 0 with r >= 0: triangles without
//           area -- no dipole stands for them, the walk always descends and the leaf evaluates them exactly
// Every statement of the build and of the far / near decision is rounded on its own (no contraction into FMAs) for the reason given at
// tri_intersect: the device and the host build must take the SAME decisions from the same mesh.  (Division and sqrtf are correctly rounded
// in both builds.)  What differs between them is atan2f, i.e. the rounding of an exact term.
#pragma once
#include "dsdf_bvh.h"

namespace dsdf {

#define DSDF_WIND_REC 8            /* floats per moment record */
#define DSDF_WIND_INV_4PI 0.07957747154594767f
#define DSDF_WIND_GROW 1.000001f   /* every computed radius is grown by 8 ulps: the roundings of |p - c| and of the sum over the levels */

DSDF_HD size_t winding_moment_floats(int n_tri) { return (size_t)2 * DSDF_WIND_REC * bvh_leaves(n_tri); }

DSDF_HD V3 cross_unfused(V3 a, V3 b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
DSDF_HD float dist_unfused(V3 a, V3 b) {
    const V3 d = mk(a.x - b.x, a.y - b.y, a.z - b.z);
    return sqrtf(dot_unfused(d, d));
}

// ---- the solid angle of one triangle, written once (k_mesh_winding, the tree walk, the host tests) --------------------------------
// Van Oosterom & Strackee: with a, b, c = p0 - x, p1 - x, p2 - x,
//   Omega = 2 atan2(a . (b x c), |a||b||c| + (a . b)|c| + (b . c)|a| + (c . a)|b|),
// positive when x is on the side the geometric normal (p1 - p0) x (p2 - p0) points AWAY from: the inside of an outward-oriented closed mesh
// sums to +4 pi.  The triple product is taken as a . (e1 x e2), the same number ((b - a) x (c - a) = b x c - b x a - a x c, and a is
// orthogonal to the last two): the edges do not depend on x, so a triangle without area has a determinant of (nearly) 0 for EVERY x and
// contributes 0 off its line, and close to a large triangle the product does not cancel.  A point on the triangle gives det = +-0 and a
// denominator <= 0: +-2 pi or 0, finite; no accuracy is claimed there.
DSDF_HD float tri_solid_angle(const float *p, V3 x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const V3 a = mk(p[0] - x.x, p[1] - x.y, p[2] - x.z), b = mk(p[3] - x.x, p[4] - x.y, p[5] - x.z), c = mk(p[6] - x.x, p[7] - x.y, p[8] - x.z);
    const V3 e1 = mk(p[3] - p[0], p[4] - p[1], p[5] - p[2]), e2 = mk(p[6] - p[0], p[7] - p[1], p[8] - p[2]);
    const float det = dot_unfused(a, cross_unfused(e1, e2));
    const float la = sqrtf(dot_unfused(a, a)), lb = sqrtf(dot_unfused(b, b)), lc = sqrtf(dot_unfused(c, c));
    const float den = la * lb * lc + dot_unfused(a, b) * lc + dot_unfused(b, c) * la + dot_unfused(c, a) * lb;
    return 2.f * atan2f(det, den);
}

// ---- moments: the statements of one node, called per thread by the kernels and serially by the host tests --------------------------
DSDF_HD float *winding_record(float *mom, uint32_t heap) { return mom + (size_t)DSDF_WIND_REC * (heap + 1u); }

DSDF_HD void winding_store(float *rec, V3 N, V3 c, float r, float A) {
    rec[0] = N.x; rec[1] = N.y; rec[2] = N.z; rec[3] = c.x; rec[4] = c.y; rec[5] = c.z; rec[6] = r; rec[7] = A;
}

// leaf j from its (up to) four slots of the built BVH; leaf 0 also writes the 8 floats in front of the root's record
DSDF_HD void winding_leaf_moments(const float *bvh, float *mom, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const BvhView B = bvh_view(bvh);
    if (j == 0) for (int k = 0; k < DSDF_WIND_REC; ++k) mom[k] = k == 0 ? i2f(B.L) : 0.f;
    V3 N = mk(0.f, 0.f, 0.f), S = mk(0.f, 0.f, 0.f), M = mk(0.f, 0.f, 0.f);
    float A = 0.f;
    int cnt = 0;
    for (int k = 0; k < DSDF_BVH_LEAF; ++k) {
        float p[DSDF_BVH_SLOT];
        bvh_load_slot(B, DSDF_BVH_LEAF * j + k, p);
        if (f2i(p[9]) < 0) break;                // (slots fill from the left)
        const V3 n = cross_unfused(mk(p[3] - p[0], p[4] - p[1], p[5] - p[2]), mk(p[6] - p[0], p[7] - p[1], p[8] - p[2]));
        const V3 h = mk(0.5f * n.x, 0.5f * n.y, 0.5f * n.z);
        const float At = sqrtf(dot_unfused(h, h));
        const V3 g = mk((p[0] + p[3] + p[6]) * (1.f / 3.f), (p[1] + p[4] + p[7]) * (1.f / 3.f), (p[2] + p[5] + p[8]) * (1.f / 3.f));
        N = mk(N.x + h.x, N.y + h.y, N.z + h.z);
        S = mk(S.x + At * g.x, S.y + At * g.y, S.z + At * g.z);
        M = mk(M.x + g.x, M.y + g.y, M.z + g.z);
        A = A + At;
        ++cnt;
    }
    float *rec = winding_record(mom, (uint32_t)(B.L - 1 + j));
    if (cnt == 0) { winding_store(rec, mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 0.f), -1.f, 0.f); return; }
    const bool area = A > 0.f && A < INFINITY;
    const V3 c = area ? mk(S.x / A, S.y / A, S.z / A) : mk(M.x / (float)cnt, M.y / (float)cnt, M.z / (float)cnt);
    float r = 0.f;
    for (int k = 0; k < cnt; ++k) {
        float p[DSDF_BVH_SLOT];
        bvh_load_slot(B, DSDF_BVH_LEAF * j + k, p);
        for (int v = 0; v < 3; ++v) r = fmaxf(r, dist_unfused(mk(p[3 * v], p[3 * v + 1], p[3 * v + 2]), c));
    }
    winding_store(rec, N, c, r * DSDF_WIND_GROW, area ? A : 0.f);
}

// inner node i (its children's records are final): N and A add up, c is the area-weighted mean of the children's, and
// r = max over the children of |c_child - c| + r_child, which is conservative (it only costs descents)
DSDF_HD void winding_node_moments(float *mom, uint32_t i) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float *k0 = winding_record(mom, 2u * i + 1u), *k1 = k0 + DSDF_WIND_REC;
    float *rec = winding_record(mom, i);
    const bool e0 = k0[6] < 0.f, e1 = k1[6] < 0.f;
    if (e0 && e1) { winding_store(rec, mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 0.f), -1.f, 0.f); return; }
    if (e0 || e1) { const float *k = e0 ? k1 : k0; for (int a = 0; a < DSDF_WIND_REC; ++a) rec[a] = k[a]; return; }
    const V3 c0 = mk(k0[3], k0[4], k0[5]), c1 = mk(k1[3], k1[4], k1[5]);
    const float A0 = k0[7], A1 = k1[7], A = A0 + A1;
    const bool area = A > 0.f && A < INFINITY;
    const float w0 = area ? A0 : 1.f, w1 = area ? A1 : 1.f, ws = area ? A : 2.f;
    const V3 c = mk((w0 * c0.x + w1 * c1.x) / ws, (w0 * c0.y + w1 * c1.y) / ws, (w0 * c0.z + w1 * c1.z) / ws);
    const float r = fmaxf(dist_unfused(c0, c) + k0[6], dist_unfused(c1, c) + k1[6]);
    winding_store(rec, mk(k0[0] + k1[0], k0[1] + k1[1], k0[2] + k1[2]), c, r * DSDF_WIND_GROW, area ? A : 0.f);
}

// ---- the walk ----------------------------------------------------------------------------------------------------------------------
struct WindRec { V3 N, c; float r, A; };
DSDF_HD WindRec winding_load(const float *mom, uint32_t i1) {           // i1 = heap index + 1
    WindRec R;
#if defined(__HIP_DEVICE_COMPILE__)
    // one 32-byte record = two 16-byte loads issued together.  The fields are used under different conditions, and the compiler would
    // otherwise sink four dependent loads of the same line into the branches (r, then A, then c, then N): the empty asm pins both loads here.
    const bvh_f32x4 *q = reinterpret_cast<const bvh_f32x4 *>(mom + (size_t)DSDF_WIND_REC * i1);
    bvh_f32x4 a = q[0], b = q[1];
    asm volatile("" : "+v"(a), "+v"(b));
    R.N = mk(a.x, a.y, a.z); R.c = mk(a.w, b.x, b.y); R.r = b.z; R.A = b.w;
#else
    const float *q = mom + (size_t)DSDF_WIND_REC * i1;
    R.N = mk(q[0], q[1], q[2]); R.c = mk(q[3], q[4], q[5]); R.r = q[6]; R.A = q[7];
#endif
    return R;
}

// the exact terms of leaf j.  All four slots are evaluated and an empty one is deselected (its corners are 0: the term is 0 anyway), so
// that the twelve loads of a leaf are independent of each other instead of waiting for the index of the slot before.
DSDF_HD float winding_leaf(const BvhView &B, int j, V3 x) {
    float s = 0.f;
    for (int k = 0; k < DSDF_BVH_LEAF; ++k) {
        float p[DSDF_BVH_SLOT];
        bvh_load_slot(B, DSDF_BVH_LEAF * j + k, p);
        const float omega = tri_solid_angle(p, x);
        s += f2i(p[9]) >= 0 ? omega : 0.f;
    }
    return s;
}

// w(x) by a depth-first walk of the heap, left child first, without a stack: with the 1-based index i1 the children of a node are 2 i1
// and 2 i1 + 1, and the node that follows a finished subtree is (i1 + 1) with its trailing zero bits shifted out -- up while the node is a
// right child, then the sibling; 1 = back at the root: done.  The state is one register, and the order of the terms is the same for
// every point and build.  At a node: empty -> skip; with area and |c - x|^2 > beta^2 r^2 -> the dipole N . (c - x) / (4 pi |c - x|^3)
// stands for the whole subtree; a leaf -> its triangles exactly; otherwise descend.  beta = +inf makes the bound inf (or NaN for r = 0),
// which no distance exceeds: the exact sum.  The caller refuses beta < 1 (a point INSIDE the ball of a subtree is no far field).
DSDF_HD float bvh_winding(const BvhView &B, const float *mom, V3 x, float beta) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const uint32_t L = (uint32_t)B.L;
    float s = 0.f;
    uint32_t i1 = 1u;
    for (;;) {
        const WindRec R = winding_load(mom, i1);
        bool down = false;
        if (R.r >= 0.f) {
            const V3 d = mk(R.c.x - x.x, R.c.y - x.y, R.c.z - x.z);
            const float d2 = dot_unfused(d, d), br = beta * R.r;
            if (R.A > 0.f && d2 > br * br) s += dot_unfused(R.N, d) / (d2 * sqrtf(d2));
            else if (i1 >= L) s += winding_leaf(B, (int)(i1 - L), x);
            else down = true;
        }
        if (down) { i1 = 2u * i1; continue; }
        const uint32_t t = i1 + 1u;
        i1 = t >> __builtin_ctz(t);
        if (i1 == 1u) break;
    }
    return s * DSDF_WIND_INV_4PI;
}

}  // namespace dsdf

#if defined(__HIPCC__)
// =========================================================================================================================
// Kernels and entry points (fail / launch of dsdf_kernels.hip and the tile loop of dsdf_mesh.h are in scope).
// =========================================================================================================================

// The exact sum, N-body style like k_mesh_closest (mesh_for_each_triangle, dsdf_mesh.h): every thread adds the solid angles of the staged
// triangles at its point, in index order.  atan2f is the expensive instruction of the inner loop (~40 VALU instructions of its own
// against ~45 for the rest of the term).
__global__ __launch_bounds__(256) void k_mesh_winding(const float *__restrict__ tri, int n_tri, const float *__restrict__ pts, int64_t n,
                                                      float *__restrict__ w_out) {
    __shared__ float tile[DSDF_MESH_TILE * 9];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = i < n;
    V3 x = mk(0.f, 0.f, 0.f);
    if (on) x = mk(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    float s = 0.f;
    mesh_for_each_triangle(tri, n_tri, tile, [&s, x](const float *p, int) { s += tri_solid_angle(p, x); });
    if (on) w_out[i] = s * DSDF_WIND_INV_4PI;
}

__global__ __launch_bounds__(256) void k_wind_leaves(const float *__restrict__ bvh, float *__restrict__ mom, int n_leaves) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_leaves && f2i(bvh[1]) == n_leaves) winding_leaf_moments(bvh, mom, j);       // (a count that is not this tree's: nothing is written)
}

// the inner nodes of one level, [first, first + count), deepest level first
__global__ __launch_bounds__(256) void k_wind_level(float *__restrict__ mom, uint32_t first, uint32_t count) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < count) winding_node_moments(mom, first + k);
}

// One lane per query point, in the caller's order: voxel-ordered points make neighbouring lanes walk the same nodes, so a node record
// (32 bytes, both children in one 64-byte line) is one cache line for most of a wave.
__global__ __launch_bounds__(256) void k_mesh_bvh_winding(const float *__restrict__ bvh, const float *__restrict__ mom, const float *__restrict__ pts,
                                                          int64_t n, float beta, float *__restrict__ w_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const BvhView B = bvh_view(bvh);
    if (f2i(mom[0]) != B.L) { w_out[i] = NAN; return; }        // the moments of another tree
    w_out[i] = bvh_winding(B, mom, mk(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]), beta);
}

extern "C" {

int dsdf_mesh_winding(const float *triangles, int n_triangles, const float *points, int64_t n, float *w_out, void *stream) {
    if (n == 0) return DSDF_OK;
    if (!triangles || n_triangles < 1 || !points || !w_out || n < 0) return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_winding: bad argument");
    return launch_lanes("k_mesh_winding", k_mesh_winding, n, (hipStream_t)stream, triangles, n_triangles,
                  points, n, w_out);
}

size_t dsdf_mesh_bvh_moments_size(int n_triangles) { return n_triangles < 1 ? 0 : winding_moment_floats(n_triangles); }

int dsdf_mesh_bvh_moments(const float *bvh, int n_triangles, float *moments_out, void *stream) {
    if (!bvh || n_triangles < 1 || !moments_out) return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_bvh_moments: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int L = bvh_leaves(n_triangles);
    int rc;
    if ((rc = launch_lanes("k_wind_leaves", k_wind_leaves, L, st, bvh, moments_out, L))) return rc;
    for (uint32_t count = (uint32_t)L >> 1; count >= 1; count >>= 1)       // nodes [count - 1, 2 count - 1), the root included
        if ((rc = launch_lanes("k_wind_level", k_wind_level, count, st, moments_out, count - 1u, count))) return rc;
    return DSDF_OK;
}

int dsdf_mesh_bvh_winding(const float *bvh, const float *moments, const float *points, int64_t n, float beta, float *w_out, void *stream) {
    if (n == 0) return DSDF_OK;
    if (!bvh || !moments || !points || !w_out || n < 0) return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_bvh_winding: bad argument");
    if (!(beta >= 1.f)) return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_bvh_winding: beta must be >= 1 (+inf: the exact sum)");
    return launch_lanes("k_mesh_bvh_winding", k_mesh_bvh_winding, n, (hipStream_t)stream, bvh, moments,
                  points, n, beta, w_out);
}

}  // extern "C"
#endif  // __HIPCC__
