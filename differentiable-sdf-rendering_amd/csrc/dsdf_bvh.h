// dsdf_bvh.h -- a bounding-volume hierarchy over a triangle soup: layout, builder, traversal, and the primal render of a mesh
// on top of it (reference images of mesh scenes: python/optimize.py:11-40 renders them from the scene's mesh with Mitsuba).
//
// Two parts.  The first is host/device inline arithmetic (the triangle test, the slab test, the builder's per-element
// statements, the stackless traversal, what the loops over all triangles of dsdf_mesh.h keep per ray and per point, what a
// closest-point query stores) and compiles with any C++ compiler: the host-side tests run exactly these statements.
// The second, under __HIPCC__, holds the kernels and the C-ABI entry points and is included at the end of dsdf_kernels.hip.
//
// LAYOUT (ABI, include/dsdf.h).  An implicit COMPLETE binary tree in one caller-owned buffer of floats.  T triangles, 4 per
// leaf, L = the smallest power of two >= ceil(T / 4) leaves, L - 1 inner nodes in heap order (children of i: 2 i + 1, 2 i + 2;
// leaf j is heap node L - 1 + j):
//   [0, 16)              header: int T, int L, int has_normals, float margin, float lo[3], float hi[3] (the mesh AABB), 6 x 0
//   [16, 16 L)           inner node i at 16 + 16 i: child 0 lo.xyz hi.xyz, child 1 lo.xyz hi.xyz, 4 x 0  -- one 64-byte fetch
//   [16 L, 64 L)         triangle slot s at 16 L + 12 s (leaf j owns slots 4 j .. 4 j + 3, filled from the left, in the order of
//                        the caller's permutation): p0 p1 p2, int original index (-1: empty slot), 2 x 0
//   [64 L, 100 L)        only with normals: slot s at 64 L + 9 s: the vertex normals n0 n1 n2 of that triangle
// A leaf's box lives in its parent like any child's; L = 1 has no box at all (its one leaf is always tested).  Empty leaves
// (and inner nodes over nothing but empty leaves) have the inverted box lo = +inf, hi = -inf, which the slab test refuses.
//
// BOXES are conservative towards the TRIANGLE TEST, not towards the exact triangle: the traversal must return bit for bit what
// the loop over all triangles returns, so a box may never cull a triangle that tri_intersect would accept at a distance inside
// the ray's window.  An accepted hit sits at a computed t whose point o + t d is within fp32 rounding of the triangle; the
// leaf boxes are therefore grown by DSDF_BVH_MARGIN x the largest extent of the mesh AABB on every side (2^-13: three
// orders of magnitude above the rounding of the slab arithmetic for origins within a few extents of the mesh, ~1 % of a
// triangle's edge at 80 k triangles on a sphere).  A triangle whose corners are (nearly) collinear has a determinant that is
// rounding noise for EVERY ray -- the loop over all triangles can accept it anywhere -- so it gets an infinite box and is
// always tested.  The window test is closed (near <= best): a triangle at exactly the best distance with a lower index wins.
//
// CLOSEST-POINT queries (tri_closest, box_dist2, bvh_closest) descend the same tree by the distance of the query point to the boxes
// and keep the same promise towards tri_closest: the bits of the loop over all triangles, for query points within roughly 100
// extents of the mesh -- the same margin against the roundings of a squared distance; the argument stands at bvh_closest.
#pragma once
#include <string.h>
#include "dsdf_math.h"

namespace dsdf {

#define DSDF_BVH_HEADER 16
#define DSDF_BVH_NODE 16
#define DSDF_BVH_LEAF 4            /* triangles per leaf */
#define DSDF_BVH_SLOT 12           /* floats per triangle slot */
#define DSDF_BVH_MARGIN 1.220703125e-4f   /* 2^-13 of the mesh AABB's largest extent */
#define DSDF_BVH_DEGENERATE 9.5367431640625e-7f   /* 2^-20: |e1 x e2|^2 <= this |e1|^2 |e2|^2 (sine below 2^-10): always tested */

DSDF_HD int f2i(float f) { int i; memcpy(&i, &f, 4); return i; }
DSDF_HD float i2f(int i) { float f; memcpy(&f, &i, 4); return f; }

DSDF_HD int bvh_leaves(int n_tri) {
    const int need = (n_tri + DSDF_BVH_LEAF - 1) / DSDF_BVH_LEAF;
    int L = 1;
    while (L < need) L <<= 1;
    return L;
}
DSDF_HD size_t bvh_floats(int n_tri, int has_normals) { return (size_t)bvh_leaves(n_tri) * (has_normals ? 100 : 64); }

struct BvhView { const float *nodes, *slots, *nrm; int T, L; };
DSDF_HD BvhView bvh_view(const float *bvh) {
    BvhView B;
    B.T = f2i(bvh[0]); B.L = f2i(bvh[1]);
    B.nodes = bvh + DSDF_BVH_HEADER;
    B.slots = bvh + (size_t)16 * B.L;
    B.nrm = f2i(bvh[2]) ? bvh + (size_t)64 * B.L : nullptr;
    return B;
}

// ---- the triangle test, written once (k_mesh_raycast, the traversal, the host tests) ------------------------------------
// Moeller-Trumbore, o + t d = p0 + u e1 + v e2, for the triangle p[0..8] = p0 p1 p2.  false: the ray is parallel to the plane
// (det == 0) or passes outside; the caller applies its distance window.  det = e1 . (d x e2) = -d . (e1 x e2): negative when
// the geometric normal (p1 - p0) x (p2 - p0) points along the ray.
// Every product and sum below is rounded on its own (no contraction into FMAs): which of the two products of `a b - c d` a
// compiler fuses depends on the code around it, and the brute-force kernel and the traversal kernel -- and the host build of the
// tests -- must compute the SAME bits from the same triangle and ray.
struct TriHit { float t, u, v, det; };
DSDF_HD float dot_unfused(V3 a, V3 b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return a.x * b.x + a.y * b.y + a.z * b.z;
}
DSDF_HD bool tri_intersect(const float *p, V3 o, V3 d, TriHit &h) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const V3 p0 = mk(p[0], p[1], p[2]), e1 = mk(p[3] - p[0], p[4] - p[1], p[5] - p[2]), e2 = mk(p[6] - p[0], p[7] - p[1], p[8] - p[2]);
    const V3 pv = mk(d.y * e2.z - d.z * e2.y, d.z * e2.x - d.x * e2.z, d.x * e2.y - d.y * e2.x);
    const float det = dot_unfused(e1, pv);
    if (det == 0.f) return false;
    const float inv = 1.f / det;
    const V3 tv = o - p0;
    const float u = dot_unfused(tv, pv) * inv;
    const V3 qv = mk(tv.y * e1.z - tv.z * e1.y, tv.z * e1.x - tv.x * e1.z, tv.x * e1.y - tv.y * e1.x);
    const float v = dot_unfused(d, qv) * inv;
    const float t = dot_unfused(e2, qv) * inv;
    h.t = t; h.u = u; h.v = v; h.det = det;
    return u >= 0.f && v >= 0.f && u + v <= 1.f;
}

// What the loop over all triangles keeps of a ray (k_mesh_raycast, the host tests): the nearest hit beyond t_min.  Strict `<` in index
// order, so the lowest index wins a tie -- the promise bvh_leaf keeps towards this loop.  back: det = e1 . (d x e2) = -d . (e1 x e2) is
// negative when the normal points along the ray.
struct RayBest { float t; int back, prim; };                        // prim: -1 = none, t = inf
DSDF_HD void ray_best_init(RayBest &b) { b.t = INFINITY; b.back = 0; b.prim = -1; }
DSDF_HD void ray_best_update(RayBest &b, const float *p, V3 o, V3 d, float t_min, int idx) {
    TriHit h;
    if (tri_intersect(p, o, d, h) && h.t > t_min && h.t < b.t) { b.t = h.t; b.back = h.det < 0.f ? 1 : 0; b.prim = idx; }
}

// ---- slab test ---------------------------------------------------------------------------------------------------------
// One axis: the ray is inside [lo, hi] for t in [min(ta, tb), max(ta, tb)].  A direction component of 0 (1 / d = +-inf; also a
// denormal one) makes (lo - o) * inv the NaN 0 * inf exactly when the origin lies ON a slab plane -- mesh_to_sdf casts
// (0, +-1, 0) rays from voxel centres on the symmetry planes of a mesh -- so that case is decided by comparison: the whole line
// when lo <= o <= hi, nothing otherwise.
struct BvhRay { V3 o, d, inv; };
DSDF_HD BvhRay bvh_ray(V3 o, V3 d) { BvhRay r; r.o = o; r.d = d; r.inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z); return r; }

DSDF_HD void slab_axis(float lo, float hi, float o, float inv, float &tnear, float &tfar) {
    const float a = lo - o, b = hi - o;
    float ta = a * inv, tb = b * inv;
    if (fabsf(inv) == INFINITY) { ta = a <= 0.f ? -INFINITY : INFINITY; tb = b >= 0.f ? INFINITY : -INFINITY; }
    tnear = fmaxf(tnear, fminf(ta, tb));
    tfar = fminf(tfar, fmaxf(ta, tb));
}
// box b = lo.xyz hi.xyz against the ray's window [t0, t1] (closed); tnear: where the ray enters (the order of the descent)
DSDF_HD bool box_hit(const float *b, const BvhRay &r, float t0, float t1, float &tnear) {
    float tn = t0, tf = t1;
    slab_axis(b[0], b[3], r.o.x, r.inv.x, tn, tf);
    slab_axis(b[1], b[4], r.o.y, r.inv.y, tn, tf);
    slab_axis(b[2], b[5], r.o.z, r.inv.z, tn, tf);
    tnear = tn;
    return tn <= tf && b[0] <= b[3];           // (an inverted box would swap its slabs under min / max: refused by name)
}

// ---- builder: the statements of one element, called per thread by the kernels and serially by the host tests ------------
// 30-bit Morton code of a triangle's centroid inside the mesh AABB
DSDF_HD uint32_t morton_spread(uint32_t v) {
    v = (v | (v << 16)) & 0x030000FFu; v = (v | (v << 8)) & 0x0300F00Fu; v = (v | (v << 4)) & 0x030C30C3u; v = (v | (v << 2)) & 0x09249249u;
    return v;
}
DSDF_HD int32_t bvh_morton(const float *p, const float lo[3], const float hi[3]) {
    uint32_t q[3];
    for (int k = 0; k < 3; ++k) {
        const float c = (p[k] + p[3 + k] + p[6 + k]) * (1.f / 3.f), ext = hi[k] - lo[k];
        const float f = ext > 0.f ? (c - lo[k]) / ext * 1024.f : 0.f;
        q[k] = (uint32_t)fminf(fmaxf(f, 0.f), 1023.f);
    }
    return (int32_t)((morton_spread(q[0]) << 2) | (morton_spread(q[1]) << 1) | morton_spread(q[2]));
}

DSDF_HD float bvh_margin(const float lo[3], const float hi[3]) {
    return DSDF_BVH_MARGIN * fmaxf(hi[0] - lo[0], fmaxf(hi[1] - lo[1], hi[2] - lo[2]));
}
DSDF_HD void bvh_write_header(float *bvh, int n_tri, int has_normals, const float lo[3], const float hi[3]) {
    bvh[0] = i2f(n_tri); bvh[1] = i2f(bvh_leaves(n_tri)); bvh[2] = i2f(has_normals ? 1 : 0); bvh[3] = bvh_margin(lo, hi);
    for (int k = 0; k < 3; ++k) { bvh[4 + k] = lo[k]; bvh[7 + k] = hi[k]; }
    for (int k = 10; k < DSDF_BVH_HEADER; ++k) bvh[k] = 0.f;
}

// where the box of heap node i (i >= 1) is stored: 6 floats in its parent
DSDF_HD float *bvh_box_of(float *bvh, uint32_t i) { return bvh + DSDF_BVH_HEADER + (size_t)DSDF_BVH_NODE * ((i - 1) >> 1) + 6 * ((i - 1) & 1u); }

// leaf j: gathers its (up to) four triangles [+ normals] through `order` (or in the given order) and writes its box.
// (The header must have been written.)
DSDF_HD void bvh_write_leaf(float *bvh, const float *tri, const float *nrm, const int32_t *order, int j) {
    const int T = f2i(bvh[0]), L = f2i(bvh[1]);
    const float margin = bvh[3];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < DSDF_BVH_LEAF; ++k) {
        const int s = DSDF_BVH_LEAF * j + k;
        float *slot = bvh + (size_t)16 * L + (size_t)DSDF_BVH_SLOT * s;
        const int src = s < T ? (order ? order[s] : s) : -1;
        for (int e = 0; e < 9; ++e) slot[e] = src >= 0 ? tri[(size_t)9 * src + e] : 0.f;
        slot[9] = i2f(src); slot[10] = 0.f; slot[11] = 0.f;
        if (nrm) {
            float *ns = bvh + (size_t)64 * L + (size_t)9 * s;
            for (int e = 0; e < 9; ++e) ns[e] = src >= 0 ? nrm[(size_t)9 * src + e] : 0.f;
        }
        if (src < 0) continue;
        const float *p = slot;
        const V3 e1 = mk(p[3] - p[0], p[4] - p[1], p[5] - p[2]), e2 = mk(p[6] - p[0], p[7] - p[1], p[8] - p[2]);
        const V3 c = mk(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x);
        if (!(dot(c, c) > DSDF_BVH_DEGENERATE * dot(e1, e1) * dot(e2, e2))) {       // (nearly) collinear, or not finite: always tested
            for (int a = 0; a < 3; ++a) { lo[a] = -INFINITY; hi[a] = INFINITY; }
            continue;
        }
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], fminf(p[a], fminf(p[3 + a], p[6 + a])) - margin);
            hi[a] = fmaxf(hi[a], fmaxf(p[a], fmaxf(p[3 + a], p[6 + a])) + margin);
        }
    }
    if (L == 1) return;
    float *b = bvh_box_of(bvh, (uint32_t)(L - 1 + j));
    for (int a = 0; a < 3; ++a) { b[a] = lo[a]; b[3 + a] = hi[a]; }
    if (j & 1) { float *pad = b + 6; for (int a = 0; a < 4; ++a) pad[a] = 0.f; }      // (child 1 sits in front of the node's padding)
}
// inner node i >= 1 (its children's boxes are final): their union is its own box, stored in ITS parent
DSDF_HD void bvh_fit_node(float *bvh, uint32_t i) {
    const float *n = bvh + DSDF_BVH_HEADER + (size_t)DSDF_BVH_NODE * i;
    float *b = bvh_box_of(bvh, i);
    for (int a = 0; a < 3; ++a) { b[a] = fminf(n[a], n[6 + a]); b[3 + a] = fmaxf(n[3 + a], n[9 + a]); }
    if (!(i & 1u)) { float *pad = b + 6; for (int a = 0; a < 4; ++a) pad[a] = 0.f; }
}

// ---- traversal ---------------------------------------------------------------------------------------------------------
// One ray, no stack: an ordered descent (the child the ray enters first) that remembers in one bit per level whether the
// other child is still owed.  With heap indices a pop is arithmetic -- the deepest owed level k below the current node, the
// ancestor at depth k + 1 is ((i + 1) >> (depth - k - 1)) - 1, the owed node its sibling -- so the state is three registers
// (a runtime-indexed per-lane stack would live in scratch memory).  Depth <= 32 by construction (L <= 2^29).
struct BvhHit { float t; int prim, slot; float u, v, det; };       // prim: original triangle index, -1 = none

struct GlobalNodes {
    const float *nodes;
    DSDF_HD void load(uint32_t i, float nd[12]) const {
#if defined(__HIP_DEVICE_COMPILE__)
        const float4 *q = reinterpret_cast<const float4 *>(nodes + (size_t)DSDF_BVH_NODE * i);
        const float4 a = q[0], b = q[1], c = q[2];
        nd[0] = a.x; nd[1] = a.y; nd[2] = a.z; nd[3] = a.w; nd[4] = b.x; nd[5] = b.y; nd[6] = b.z; nd[7] = b.w;
        nd[8] = c.x; nd[9] = c.y; nd[10] = c.z; nd[11] = c.w;
#else
        for (int k = 0; k < 12; ++k) nd[k] = nodes[(size_t)DSDF_BVH_NODE * i + k];
#endif
    }
};

DSDF_HD void bvh_load_slot(const BvhView &B, int s, float p[DSDF_BVH_SLOT]) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float4 *q = reinterpret_cast<const float4 *>(B.slots + (size_t)DSDF_BVH_SLOT * s);
    const float4 a = q[0], b = q[1], c = q[2];
    p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w; p[4] = b.x; p[5] = b.y; p[6] = b.z; p[7] = b.w;
    p[8] = c.x; p[9] = c.y; p[10] = c.z; p[11] = c.w;
#else
    for (int k = 0; k < DSDF_BVH_SLOT; ++k) p[k] = B.slots[(size_t)DSDF_BVH_SLOT * s + k];
#endif
}

// the triangles of leaf j against the window (t_min, hit.t]: on equal t the lower original index wins, which is what the
// strict `<` of a loop in index order gives.  ANY: the first triangle inside (t_min, hit.t) ends the query.
template <bool ANY>
DSDF_HD bool bvh_leaf(const BvhView &B, int j, V3 o, V3 d, float t_min, BvhHit &hit) {
    for (int k = 0; k < DSDF_BVH_LEAF; ++k) {
        const int s = DSDF_BVH_LEAF * j + k;
        float p[DSDF_BVH_SLOT];
        bvh_load_slot(B, s, p);
        const int idx = f2i(p[9]);
        if (idx < 0) break;                      // (slots fill from the left)
        TriHit h;
        if (!tri_intersect(p, o, d, h) || !(h.t > t_min)) continue;
        if (h.t < hit.t || (!ANY && h.t == hit.t && idx < hit.prim)) {
            hit.t = h.t; hit.prim = idx; hit.slot = s; hit.u = h.u; hit.v = h.v; hit.det = h.det;
            if (ANY) return true;
        }
    }
    return false;
}

// Closest hit with t_min < t < t_max (ANY: whether there is one).  hit.prim = -1 and hit.t = t_max when there is none.
template <bool ANY, class Nodes>
DSDF_HD bool bvh_traverse(const BvhView &B, const Nodes &N, V3 o, V3 d, float t_min, float t_max, BvhHit &hit) {
    hit.t = t_max; hit.prim = -1; hit.slot = 0; hit.u = 0.f; hit.v = 0.f; hit.det = 0.f;
    const uint32_t inner = (uint32_t)B.L - 1u;
    if (inner == 0u) { bvh_leaf<ANY>(B, 0, o, d, t_min, hit); return hit.prim >= 0; }
    const BvhRay r = bvh_ray(o, d);
    uint32_t i = 0;
    int depth = 0;
    uint64_t owed = 0;
    for (;;) {
        float nd[12], n0, n1;
        N.load(i, nd);
        const bool h0 = box_hit(nd, r, t_min, hit.t, n0), h1 = box_hit(nd + 6, r, t_min, hit.t, n1);
        bool down = h0 || h1;
        if (down) {
            if (h0 && h1) owed |= (uint64_t)1 << depth;
            i = 2u * i + 1u + ((h1 && (!h0 || n1 < n0)) ? 1u : 0u);
            ++depth;
        }
        for (;;) {
            if (down) {
                if (i < inner) break;
                if (bvh_leaf<ANY>(B, (int)(i - inner), o, d, t_min, hit) && ANY) return true;
            }
            const uint64_t m = owed & (((uint64_t)1 << depth) - 1u);
            if (m == 0) return hit.prim >= 0;
            const int k = 63 - __builtin_clzll(m);
            owed &= ~((uint64_t)1 << k);
            const uint32_t a = ((i + 1u) >> (depth - k - 1)) - 1u;
            i = ((a - 1u) ^ 1u) + 1u;
            depth = k + 1;
            down = true;
        }
    }
}

// ---- closest point -------------------------------------------------------------------------------------------------------
// The point of the triangle p[0..8] = p0 p1 p2 nearest to x, as q = p0 + u e1 + v e2 with u, v >= 0, u + v <= 1, and d2 = |x - q|^2.
// The minimum is attained in the face, on an edge or at a corner; instead of deciding the region first, every candidate is
// evaluated and the nearest kept: the clamped foot on each of the three edges (a corner is a clamped foot) and, when it falls
// inside, the foot in the plane.  d2 is ALWAYS |x - (p0 + u e1 + v e2)|^2 of the (u, v) kept, the distance to an actual point of the
// triangle -- so a candidate that rounding admits or refuses wrongly costs the difference between two nearly equal distances,
// never a wrong one, and a degenerate triangle needs no threshold: collinear corners have no plane (nn == 0, or a foot that is
// not finite or not inside) and leave the three edges, whose union is the longest one; three equal corners leave p0.  No division
// sees a zero: an edge parameter divides only when 0 < w . e < e . e, the plane foot only when nn > 0.
// Every product and sum is rounded on its own, for the reason given at tri_intersect: k_mesh_closest, the traversal and the host
// build must compute the same bits.  A NaN in x makes every d2 NaN, which no comparison of the callers accepts.
struct TriClosest { float d2, u, v; };
DSDF_HD float edge_param(V3 e, V3 w) {           // the foot of w on the segment 0 .. e, as a fraction of e; a zero edge is its start
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float we = dot_unfused(w, e), ee = dot_unfused(e, e);
    if (!(we > 0.f)) return 0.f;
    if (we >= ee) return 1.f;
    return we / ee;
}
DSDF_HD void tri_closest_try(V3 e1, V3 e2, V3 w, float u, float v, bool first, TriClosest &c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const V3 r = mk(w.x - (u * e1.x + v * e2.x), w.y - (u * e1.y + v * e2.y), w.z - (u * e1.z + v * e2.z));
    const float d2 = dot_unfused(r, r);
    if (first || d2 < c.d2) { c.d2 = d2; c.u = u; c.v = v; }
}
DSDF_HD void tri_closest(const float *p, V3 x, TriClosest &c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const V3 e1 = mk(p[3] - p[0], p[4] - p[1], p[5] - p[2]), e2 = mk(p[6] - p[0], p[7] - p[1], p[8] - p[2]);
    const V3 w = mk(x.x - p[0], x.y - p[1], x.z - p[2]);
    tri_closest_try(e1, e2, w, edge_param(e1, w), 0.f, true, c);                          // p0 p1
    tri_closest_try(e1, e2, w, 0.f, edge_param(e2, w), false, c);                         // p0 p2
    const float s = edge_param(mk(e2.x - e1.x, e2.y - e1.y, e2.z - e1.z), mk(w.x - e1.x, w.y - e1.y, w.z - e1.z));
    tri_closest_try(e1, e2, w, 1.f - s, s, false, c);                                     // p1 p2
    const V3 n = mk(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x);
    const float nn = dot_unfused(n, n);
    if (nn > 0.f) {
        const V3 a = mk(w.y * e2.z - w.z * e2.y, w.z * e2.x - w.x * e2.z, w.x * e2.y - w.y * e2.x);      // w x e2
        const V3 b = mk(e1.y * w.z - e1.z * w.y, e1.z * w.x - e1.x * w.z, e1.x * w.y - e1.y * w.x);      // e1 x w
        const float u = dot_unfused(a, n) / nn, v = dot_unfused(b, n) / nn;
        if (u >= 0.f && v >= 0.f && u + v <= 1.f) tri_closest_try(e1, e2, w, u, v, false, c);
    }
}
// q = p0 + u e1 + v e2, rounded the same way everywhere
DSDF_HD V3 tri_point(const float *p, float u, float v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return mk(p[0] + (u * (p[3] - p[0]) + v * (p[6] - p[0])), p[1] + (u * (p[4] - p[1]) + v * (p[7] - p[1])),
              p[2] + (u * (p[5] - p[2]) + v * (p[8] - p[2])));
}

// Squared distance of x to the box b = lo.xyz hi.xyz: the sum over the axes of max(lo - x, 0, x - hi)^2.  From the layout: the
// inverted box of an empty leaf (lo = +inf, hi = -inf) gives max(+inf, 0, +inf)^2 = +inf, which bvh_closest never enters; the
// infinite box of a (nearly) collinear triangle (lo = -inf, hi = +inf) gives max(-inf, 0, -inf)^2 = 0 and is always entered.
// (fmaxf drops a NaN operand: a NaN query is at distance 0 of every box, visits every leaf and accepts nothing.)
DSDF_HD float box_dist2(const float *b, V3 x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float dx = fmaxf(fmaxf(b[0] - x.x, 0.f), x.x - b[3]), dy = fmaxf(fmaxf(b[1] - x.y, 0.f), x.y - b[4]),
                dz = fmaxf(fmaxf(b[2] - x.z, 0.f), x.z - b[5]);
    return dx * dx + dy * dy + dz * dz;
}

// CONSERVATIVE towards tri_closest, as the ray boxes are towards tri_intersect: the traversal must return bit for bit what the
// loop over all triangles returns, so the fp32 box_dist2 of a box must not exceed the fp32 d2 of any triangle inside it.  In
// exact arithmetic the distance to a box is at most the distance to anything inside; the leaf boxes are grown by the margin
// m = 2^-13 ext on every side, which takes at least g m off the squared distance on an axis where the point is a gap g > m away
// (and a point within m of the box on every axis is at distance 0): about 1e-4 ext d for a point at distance d.  Against that
// stand the roundings: d2 is a sum of squares of differences of coordinates of size R = |x| + ext, each off by ~1e-7 R, so d2 is
// off by ~1e-7 (d^2 + d R), on either side.  The margin covers it while 1e-4 ext > ~1e-6 d, i.e. for query points within roughly
// 100 extents of the mesh; the tests stay inside 10.  Beyond that range the result is still the distance to some triangle, only
// not necessarily the bits of the loop.
struct BvhClosest { float d2; int prim, slot; float u, v; };        // prim: original triangle index, -1 = none within max_d2
// every search -- the descent, the loop over all triangles -- starts from nothing found within the bound (closest_bound)
DSDF_HD void closest_init(BvhClosest &r, float max_d2) { r.d2 = max_d2; r.prim = -1; r.slot = 0; r.u = 0.f; r.v = 0.f; }
// closed at the starting bound, and on equal d2 the lower original index wins: what `<` gives a loop in index order
DSDF_HD void closest_update(BvhClosest &r, const TriClosest &c, int idx, int s) {
    if ((c.d2 < r.d2 || (c.d2 == r.d2 && (r.prim < 0 || idx < r.prim))) && c.d2 < INFINITY) { r.d2 = c.d2; r.prim = idx; r.slot = s; r.u = c.u; r.v = c.v; }
}
DSDF_HD void bvh_closest_leaf(const BvhView &B, int j, V3 x, BvhClosest &r) {
    for (int k = 0; k < DSDF_BVH_LEAF; ++k) {
        const int s = DSDF_BVH_LEAF * j + k;
        float p[DSDF_BVH_SLOT];
        bvh_load_slot(B, s, p);
        const int idx = f2i(p[9]);
        if (idx < 0) break;                      // (slots fill from the left)
        TriClosest c;
        tri_closest(p, x, c);
        closest_update(r, c, idx, s);
    }
}
// The descent of bvh_traverse -- the nearer child first, one owed bit per level, a pop by heap arithmetic: three registers of state
// -- as a second loop, so that the ray path compiles to what it did.  A box is entered when box_dist2 <= r.d2 (closed: a triangle
// at exactly the best distance with a lower index still wins) and finite.
template <class Nodes>
DSDF_HD void bvh_closest(const BvhView &B, const Nodes &N, V3 x, float max_d2, BvhClosest &r) {
    closest_init(r, max_d2);
    const uint32_t inner = (uint32_t)B.L - 1u;
    if (inner == 0u) { bvh_closest_leaf(B, 0, x, r); return; }
    uint32_t i = 0;
    int depth = 0;
    uint64_t owed = 0;
    for (;;) {
        float nd[12];
        N.load(i, nd);
        const float n0 = box_dist2(nd, x), n1 = box_dist2(nd + 6, x);
        const bool h0 = n0 <= r.d2 && n0 < INFINITY, h1 = n1 <= r.d2 && n1 < INFINITY;
        bool down = h0 || h1;
        if (down) {
            if (h0 && h1) owed |= (uint64_t)1 << depth;
            i = 2u * i + 1u + ((h1 && (!h0 || n1 < n0)) ? 1u : 0u);
            ++depth;
        }
        for (;;) {
            if (down) {
                if (i < inner) break;
                bvh_closest_leaf(B, (int)(i - inner), x, r);
            }
            const uint64_t m = owed & (((uint64_t)1 << depth) - 1u);
            if (m == 0) return;
            const int k = 63 - __builtin_clzll(m);
            owed &= ~((uint64_t)1 << k);
            const uint32_t a = ((i + 1u) >> (depth - k - 1)) - 1u;
            i = ((a - 1u) ^ 1u) + 1u;
            depth = k + 1;
            down = true;
        }
    }
}
// The bound the searches start from, and the result they report, for a limit on the DISTANCE: sqrtf is monotone, so every d2 with
// sqrtf(d2) <= max_dist lies below max_dist^2 widened by a few ulps; closest_dist then applies the limit itself, closed.
DSDF_HD float closest_bound(float max_dist) { return max_dist * max_dist * (1.f + 4.76837158203125e-7f); }
DSDF_HD float closest_dist(BvhClosest &r, float max_dist) {
    const float d = sqrtf(r.d2);
    if (r.prim >= 0 && d <= max_dist) return d;
    r.prim = -1;
    return INFINITY;
}
// what every closest-point query -- both kernels, the host tests -- writes for point i from the search result and the nine floats of the
// winning triangle; every output but the distance may be null
DSDF_HD void closest_store(BvhClosest r, const float *p, float max_dist, int64_t i, float *__restrict__ dist_out, int32_t *__restrict__ prim_out,
                           float *__restrict__ point_out, float *__restrict__ bary_out) {
    dist_out[i] = closest_dist(r, max_dist);
    if (prim_out) prim_out[i] = r.prim;
    const bool found = r.prim >= 0;
    if (point_out) {
        const V3 q = found ? tri_point(p, r.u, r.v) : mk(0.f, 0.f, 0.f);
        point_out[3 * i] = q.x; point_out[3 * i + 1] = q.y; point_out[3 * i + 2] = q.z;
    }
    if (bary_out) { bary_out[2 * i] = found ? r.u : 0.f; bary_out[2 * i + 1] = found ? r.v : 0.f; }
}

// the shading normal of a hit: the interpolated vertex normals when the buffer has them, else the geometric normal
DSDF_HD V3 bvh_normal(const BvhView &B, const BvhHit &h) {
    V3 n;
    if (B.nrm) {
        const float *q = B.nrm + (size_t)9 * h.slot;
        const float w = 1.f - h.u - h.v;
        n = mk(w * q[0] + h.u * q[3] + h.v * q[6], w * q[1] + h.u * q[4] + h.v * q[7], w * q[2] + h.u * q[5] + h.v * q[8]);
    } else {
        float p[DSDF_BVH_SLOT];
        bvh_load_slot(B, h.slot, p);
        const V3 e1 = mk(p[3] - p[0], p[4] - p[1], p[5] - p[2]), e2 = mk(p[6] - p[0], p[7] - p[1], p[8] - p[2]);
        n = mk(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x);
    }
    return n * (1.f / sqrtf(dot(n, n)));
}

// the reflectance of a hit from the colours per triangle corner (n_triangles x 9: rgb of p0, p1, p2, in the CALLER's triangle order --
// indexed by the original index, not by the slot): the barycentric interpolation (1 - u - v) c0 + u c1 + v c2
DSDF_HD void bvh_corner_color(const float *corner_colors, const BvhHit &h, float rgb[3]) {
    const float *q = corner_colors + (size_t)9 * h.prim;
    const float w = 1.f - h.u - h.v;
    for (int c = 0; c < 3; ++c) rgb[c] = w * q[c] + h.u * q[3 + c] + h.v * q[6 + c];
}

}  // namespace dsdf

#if defined(__HIPCC__)
// =========================================================================================================================
// Kernels and entry points (dsdf_kernels.hip includes this file last: fail / launch / the film and lane code are in scope).
// =========================================================================================================================

// The top of the heap is a contiguous prefix of the node array, so a block can stage the first DSDF_BVH_LDS_NODES nodes in LDS
// (255 = levels 0 .. 7, 16 KB) and serve every ray's first box tests from there.  Measured (profiles/mesh_bvh.md: 1 M random and
// 1 M camera rays, 5 k .. 82 k triangles, alternating builds): no difference beyond the noise -- the top of the tree is a few KB that
// every wave reads and stays in the caches -- so the default is 0, no staging; -DDSDF_BVH_LDS_NODES=255 builds it for a re-measurement.
#ifndef DSDF_BVH_LDS_NODES
#define DSDF_BVH_LDS_NODES 0
#endif

typedef float bvh_f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bvh_f32x4 bvh_lds_f32x4;      // ds_read_b128 (a generic pointer would make it a flat load)
struct StagedNodes {
    const float *nodes;
    const float4 *top;            // LDS copy of nodes [0, n_top)
    uint32_t n_top;
    __device__ __forceinline__ void load(uint32_t i, float nd[12]) const {
        if (DSDF_BVH_LDS_NODES > 0 && i < n_top) {
            const bvh_lds_f32x4 *q = (const bvh_lds_f32x4 *)(top + 4 * i);
            const bvh_f32x4 a = q[0], b = q[1], c = q[2];
            nd[0] = a.x; nd[1] = a.y; nd[2] = a.z; nd[3] = a.w; nd[4] = b.x; nd[5] = b.y; nd[6] = b.z; nd[7] = b.w;
            nd[8] = c.x; nd[9] = c.y; nd[10] = c.z; nd[11] = c.w;
        } else {
            GlobalNodes G;
            G.nodes = nodes;
            G.load(i, nd);
        }
    }
};
#define DSDF_BVH_LDS_FLOAT4 (DSDF_BVH_LDS_NODES > 0 ? 4 * DSDF_BVH_LDS_NODES : 4)
// all threads of the block call; ends with the block's barrier
__device__ __forceinline__ StagedNodes stage_nodes(const BvhView &B, float4 *top) {
    StagedNodes N;
    N.nodes = B.nodes; N.top = top;
    N.n_top = min((uint32_t)DSDF_BVH_LDS_NODES, (uint32_t)B.L - 1u);
    const float4 *src = reinterpret_cast<const float4 *>(B.nodes);
    for (uint32_t e = threadIdx.x; e < 4u * N.n_top; e += blockDim.x) top[e] = src[e];
    __syncthreads();
    return N;
}

__global__ __launch_bounds__(256) void k_mesh_bvh_raycast(const float *__restrict__ bvh, const float *__restrict__ ro, const float *__restrict__ rd,
                                                          int64_t n, float t_min, float *__restrict__ t_out, int32_t *__restrict__ back_out,
                                                          int32_t *__restrict__ prim_out) {
    __shared__ float4 top[DSDF_BVH_LDS_FLOAT4];
    const BvhView B = bvh_view(bvh);
    const StagedNodes N = stage_nodes(B, top);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 o = mk(ro[3 * i], ro[3 * i + 1], ro[3 * i + 2]), d = mk(rd[3 * i], rd[3 * i + 1], rd[3 * i + 2]);
    BvhHit h;
    bvh_traverse<false>(B, N, o, d, t_min, INFINITY, h);
    t_out[i] = h.t;
    if (back_out) back_out[i] = (h.prim >= 0 && h.det < 0.f) ? 1 : 0;
    if (prim_out) prim_out[i] = h.prim;
}

// one lane per query point
__global__ __launch_bounds__(256) void k_mesh_bvh_closest(const float *__restrict__ bvh, const float *__restrict__ pts, int64_t n, float max_dist,
                                                          float *__restrict__ dist_out, int32_t *__restrict__ prim_out,
                                                          float *__restrict__ point_out, float *__restrict__ bary_out) {
    __shared__ float4 top[DSDF_BVH_LDS_FLOAT4];
    const BvhView B = bvh_view(bvh);
    const StagedNodes N = stage_nodes(B, top);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 x = mk(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    BvhClosest r;
    bvh_closest(B, N, x, closest_bound(max_dist), r);
    float p[DSDF_BVH_SLOT];
    bvh_load_slot(B, r.slot, p);                    // (slot 0 exists in every buffer)
    closest_store(r, p, max_dist, i, dist_out, prim_out, point_out, bary_out);
}

// ---- build ---------------------------------------------------------------------------------------------------------------
// AABB of all corners by ONE block of 1024 threads (asset preparation: 100 k triangles are 3.6 MB); every thread returns it.
__device__ __forceinline__ void block_aabb(const float *__restrict__ tri, int n_tri, float lo[3], float hi[3]) {
    __shared__ float red[16][6];
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (int64_t e = threadIdx.x; e < (int64_t)n_tri * 3; e += blockDim.x)
        for (int a = 0; a < 3; ++a) { const float x = tri[3 * e + a]; lo[a] = fminf(lo[a], x); hi[a] = fmaxf(hi[a], x); }
    for (int a = 0; a < 3; ++a)
        for (int m = 32; m >= 1; m >>= 1) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], m)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], m)); }
    const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) for (int a = 0; a < 3; ++a) { red[w][a] = lo[a]; red[w][3 + a] = hi[a]; }
    __syncthreads();
    for (int a = 0; a < 3; ++a) { lo[a] = red[0][a]; hi[a] = red[0][3 + a]; }
    for (int k = 1; k < nw; ++k)
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], red[k][a]); hi[a] = fmaxf(hi[a], red[k][3 + a]); }
}

__global__ __launch_bounds__(1024) void k_mesh_morton(const float *__restrict__ tri, int n_tri, int32_t *__restrict__ codes) {
    float lo[3], hi[3];
    block_aabb(tri, n_tri, lo, hi);
    for (int t = threadIdx.x; t < n_tri; t += blockDim.x) codes[t] = bvh_morton(tri + (size_t)9 * t, lo, hi);
}

__global__ __launch_bounds__(1024) void k_bvh_header(const float *__restrict__ tri, int n_tri, int has_normals, float *__restrict__ bvh) {
    float lo[3], hi[3];
    block_aabb(tri, n_tri, lo, hi);
    if (threadIdx.x == 0) bvh_write_header(bvh, n_tri, has_normals, lo, hi);
}

__global__ __launch_bounds__(256) void k_bvh_leaves(float *__restrict__ bvh, const float *__restrict__ tri, const float *__restrict__ nrm,
                                                    const int32_t *__restrict__ order, int n_leaves) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_leaves) bvh_write_leaf(bvh, tri, nrm, order, j);
}

// the inner nodes of one level, [first, first + count), deepest level first
__global__ __launch_bounds__(256) void k_bvh_level(float *__restrict__ bvh, uint32_t first, uint32_t count) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < count) bvh_fit_node(bvh, first + k);
}

// ---- primal render of a mesh -------------------------------------------------------------------------------------------
// One lane per film sample in the reference's lane order (reparam.py:140-155): camera ray, closest hit, the primal `sample()`
// statement of the integrator with the intersection routine swapped (no warp, det = 1), re-projection of o + d, film splat.
// spp % 64 == 0: a wave is 64 samples of one pixel and reduces its 5 x 5 window before it touches memory (film_accum_wave).
// COLORS (DSDF_DIRECT only): the reflectance comes from `corner_colors` (bvh_corner_color) and S.albedo is not read; the instantiations
// without it never touch the pointer.
template <int NCH, bool COLORS>
__global__ __launch_bounds__(DSDF_BLOCK) void k_mesh_render(const float *__restrict__ bvh, const float *__restrict__ corner_colors, dsdf_params P,
                                                            ViewBatch VB, float *__restrict__ blocks, uint32_t n_lanes, ShadeArgs S) {
    __shared__ float4 top[DSDF_BVH_LDS_FLOAT4];
    __shared__ __attribute__((aligned(16))) float film_lds[DSDF_BLOCK / 64][DSDF_TROWS * DSDF_TSTRIDE];
    const ViewArgs &A = VB.v[blockIdx.y];
    float *__restrict__ block = blocks + (size_t)blockIdx.y * NCH * A.Wb * A.Hb;
    const BvhView B = bvh_view(bvh);
    const StagedNodes N = stage_nodes(B, top);
    const uint32_t t = blockIdx.x * DSDF_BLOCK + threadIdx.x;
    const bool valid = t < n_lanes;
    if (__ballot(valid) == 0) return;
    const uint32_t lane = valid ? t : n_lanes - 1;
    const Lane L = lane_setup<true>(A, P, lane);
    const V3 o = L.ray.o, d = L.ray.d;
    BvhHit h;
    const bool hit = bvh_traverse<false>(B, N, o, d, 0.f, L.ray.maxt, h);
    float vals[3] = {0.f, 0.f, 0.f};
    if (A.integrator == DSDF_SILHOUETTE) vals[0] = hit ? 1.f : 0.f;
    else if (A.integrator == DSDF_SIMPLE_SHADING) { if (hit) vals[0] = fmaxf(dot(bvh_normal(B, h), light_dir(A)), 0.f); }
    else if (!hit) {
        if (!S.hide_emitters) { vals[0] = S.env[0]; vals[1] = S.env[1]; vals[2] = S.env[2]; }
    } else {
        // sdf_direct_reparam.py:29-75 (use_mis = False): emitter sampling of the constant environment, diffuse BSDF
        DirectHit dh;
        dh.lit = false;
        dh.p = fma3(h.t, d, o);
        dh.n = bvh_normal(B, h);
        dh.g = dh.n;
        float e0, e1;
        emitter_sample(A, lane, e0, e1);
        dh.sr = spawn_shadow_ray(dh.p, dh.n, square_to_uniform_sphere(e0, e1));
        if (dot(dh.n, dh.sr.d) > 0.f && dot(dh.n, -d) > 0.f) {
            BvhHit sh;
            if (!bvh_traverse<true>(B, N, dh.sr.o, dh.sr.d, 0.f, dh.sr.maxt, sh)) {
                EmitterTerm e;
                emitter_term(S, dh, d, e);
                float alb[3]; V3 ag[3];
                if (COLORS) bvh_corner_color(corner_colors, h, alb);
                else eval_trilinear(S.albedo, dh.p, alb, ag);
#pragma unroll
                for (int c = 0; c < 3; ++c) vals[c] = (alb[c] * e.ke + e.ks) * S.env[c];
            }
        }
    }
    const Reproj rp = reproject(A.cam, P, o + d, A.W, A.H);
    if (A.spp % 64 == 0) {
        const int lid = lane_id();
        float acc[NCH][2];
#pragma unroll
        for (int c = 0; c < NCH; ++c) { acc[c][0] = 0.f; acc[c][1] = 0.f; }
        film_accum_wave<NCH>(L.px, L.py, rp.u, rp.v, vals, film_lds[threadIdx.x >> 6], lid, acc);
        film_flush_wave<NCH>(block, A, L.px, L.py, lid, acc);
    } else if (valid) splat_lane<NCH - 1>(block, A.Wb, A.Hb, rp.u, rp.v, vals, AtomicAdd());
}

extern "C" {

size_t dsdf_mesh_bvh_size(int n_triangles, int has_normals) { return n_triangles < 1 ? 0 : bvh_floats(n_triangles, has_normals); }

int dsdf_mesh_morton(const float *triangles, int n_triangles, int32_t *codes_out, void *stream) {
    if (!triangles || n_triangles < 1 || !codes_out) return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_morton: bad argument");
    return launch("k_mesh_morton", k_mesh_morton, dim3(1), dim3(1024), (hipStream_t)stream, triangles, n_triangles, codes_out);
}

int dsdf_mesh_bvh_build(const float *triangles, const float *normals, const int32_t *order, int n_triangles, float *bvh, void *stream) {
    if (!triangles || n_triangles < 1 || !bvh) return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_bvh_build: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int L = bvh_leaves(n_triangles);
    int rc;
    if ((rc = launch("k_bvh_header", k_bvh_header, dim3(1), dim3(1024), st, triangles, n_triangles, normals ? 1 : 0, bvh))) return rc;
    if ((rc = launch_lanes("k_bvh_leaves", k_bvh_leaves, L, st, bvh, triangles, normals, order, L))) return rc;
    for (uint32_t count = (uint32_t)L >> 1; count >= 2; count >>= 1)       // nodes [count - 1, 2 count - 1): the level above the last fitted one
        if ((rc = launch_lanes("k_bvh_level", k_bvh_level, count, st, bvh, count - 1u, count))) return rc;
    return DSDF_OK;
}

int dsdf_mesh_bvh_raycast(const float *bvh, const float *rays_o, const float *rays_d, int64_t n, float t_min, float *t_out,
                          int32_t *backface_out, int32_t *prim_out, void *stream) {
    if (n == 0) return DSDF_OK;
    if (!bvh || !rays_o || !rays_d || !t_out || n < 0) return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_bvh_raycast: bad argument");
    return launch_lanes("k_mesh_bvh_raycast", k_mesh_bvh_raycast, n, (hipStream_t)stream, bvh, rays_o,
                  rays_d, n, t_min, t_out, backface_out, prim_out);
}

int dsdf_mesh_bvh_closest(const float *bvh, const float *points, int64_t n, float max_dist, float *dist_out, int32_t *prim_out,
                          float *point_out, float *bary_out, void *stream) {
    if (n == 0) return DSDF_OK;
    if (!bvh || !points || !dist_out || n < 0 || !(max_dist >= 0.f)) return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_bvh_closest: bad argument");
    return launch_lanes("k_mesh_bvh_closest", k_mesh_bvh_closest, n, (hipStream_t)stream, bvh, points, n,
                  max_dist, dist_out, prim_out, point_out, bary_out);
}

size_t dsdf_mesh_render_workspace_size(int width, int height, int n_views) {
    if (width < 1 || height < 1 || n_views < 1) return 0;
    return (size_t)(n_views < DSDF_MAX_BATCH ? n_views : DSDF_MAX_BATCH) * (width + 2 * DSDF_BORDER) * (height + 2 * DSDF_BORDER) * 4 * sizeof(float);
}

// (the error texts keep the name of the call the two entry points share)
int dsdf_mesh_render_forward_colors(const float *bvh, const float *corner_colors, const dsdf_params *prm, const dsdf_camera *cams, int n_views,
                                    int width, int height, int spp, const float *offsets, const uint32_t *seeds, int integrator,
                                    const dsdf_shading *shading, float *image_out, void *workspace, size_t workspace_bytes, void *stream) {
    if (!bvh || !prm || !cams || !image_out || !workspace) return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_render_forward: null pointer argument");
    if (n_views < 1 || width < 1 || height < 1 || spp < 1) return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_render_forward: non-positive size argument");
    if (integrator != DSDF_SILHOUETTE && integrator != DSDF_SIMPLE_SHADING && integrator != DSDF_DIRECT)
        return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_render_forward: unknown integrator id");
    const bool direct = integrator == DSDF_DIRECT;
    const bool colors = direct && corner_colors;             // (the other integrators have no reflectance: the colours are ignored)
    if (direct && (!shading || (!colors && (!shading->albedo || shading->ax < 1 || shading->ay < 1 || shading->az < 1))))
        return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_render_forward: sdf_direct_reparam needs a dsdf_shading with an albedo volume"
                                          " (or, with corner colours, a dsdf_shading for the emitter)");
    if (direct && (shading->bsdf != 0 || shading->use_mis != 0))
        return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_render_forward: a mesh is rendered with the diffuse BSDF and emitter sampling only (bsdf = 0, use_mis = 0)");
    if (!offsets && !seeds) return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_render_forward: need offsets or seeds");
    const size_t Wb = width + 2 * DSDF_BORDER, Hb = height + 2 * DSDF_BORDER, nl = Wb * Hb * (size_t)spp;
    if (nl > 0x40000000ull) return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_render_forward: wavefront size exceeds 0x40000000 lanes");
    const int nch = direct ? 4 : 2;
    const size_t per_view = Wb * Hb * nch * sizeof(float);
    if (workspace_bytes < dsdf_mesh_render_workspace_size(width, height, 1))
        return fail(DSDF_ERR_WORKSPACE, "dsdf_mesh_render_forward: workspace too small (dsdf_mesh_render_workspace_size)");
    int nb = (int)(workspace_bytes / per_view);
    nb = nb < DSDF_MAX_BATCH ? nb : DSDF_MAX_BATCH;
    hipStream_t st = (hipStream_t)stream;
    ShadeArgs S;
    memset(&S, 0, sizeof(S));
    const float *emitter_u = nullptr;
    if (direct) {
        if (!colors) { S.albedo.data = shading->albedo; S.albedo.rx = shading->ax; S.albedo.ry = shading->ay; S.albedo.rz = shading->az; }
        for (int k = 0; k < 3; ++k) S.env[k] = shading->env_radiance[k];
        S.hide_emitters = shading->hide_emitters;
        emitter_u = shading->emitter_samples;
    }
    float *blocks = (float *)workspace;
    for (int v0 = 0; v0 < n_views; v0 += nb) {
        const int nv = (n_views - v0) < nb ? (n_views - v0) : nb;
        ViewBatch VB;
        for (int i = 0; i < nv; ++i) {
            const size_t v = (size_t)(v0 + i);
            VB.v[i] = make_view_args(cams[v], width, height, spp, offsets ? offsets + v * nl * 2 : nullptr, seeds ? seeds[v] : 0u, integrator,
                                     0, *prm, emitter_u ? emitter_u + v * nl * 2 : nullptr);
        }
        if (hipMemsetAsync(blocks, 0, nv * per_view, st) != hipSuccess) return fail(DSDF_ERR_LAUNCH, "dsdf_mesh_render_forward: hipMemsetAsync(film block) failed");
        int rc = launch("k_mesh_render", colors ? k_mesh_render<4, true> : (direct ? k_mesh_render<4, false> : k_mesh_render<2, false>),
                        dim3((unsigned)((nl + DSDF_BLOCK - 1) / DSDF_BLOCK), nv), dim3(DSDF_BLOCK), st, bvh, colors ? corner_colors : nullptr, *prm,
                        VB, blocks, (uint32_t)nl, S);
        if (rc) return rc;
        if ((rc = develop(blocks, nv, width, height, direct, image_out + v0 * (size_t)width * height * 3, st))) return rc;
    }
    return DSDF_OK;
}

int dsdf_mesh_render_forward(const float *bvh, const dsdf_params *prm, const dsdf_camera *cams, int n_views, int width, int height, int spp,
                             const float *offsets, const uint32_t *seeds, int integrator, const dsdf_shading *shading, float *image_out,
                             void *workspace, size_t workspace_bytes, void *stream) {
    return dsdf_mesh_render_forward_colors(bvh, nullptr, prm, cams, n_views, width, height, spp, offsets, seeds, integrator, shading, image_out,
                                           workspace, workspace_bytes, stream);
}

}  // extern "C"
#endif  // __HIPCC__
