// dsdf_components.h -- connected components of an indexed triangle mesh by a lock-free union-find over the index buffer, and the two
// per-face measures (area, signed volume term) that the binding sums per component.  Which triangles belong together: what drops the
// floaters of an optimised SDF before a mesh is written, simplified or scored.
//
// Two parts, like dsdf_simplify.h: host/device inline statements that any C++ compiler builds -- the host-side tests run exactly these,
// serially -- and, under __HIPCC__, the kernels and the C-ABI entry points (dsdf_kernels.hip includes this file after dsdf_simplify.h).
// No allocation, no synchronisation; numbering the labels 0 ... C - 1 and the per-component sums are the caller's (plumbing).
//
// CONNECTIVITY.  Two vertices are connected when a face names both: connection by shared vertex INDEX, not by shared edge (two
// triangles that touch in one vertex are one component) and not by position (a soup that repeats its vertices falls apart; the binding
// can weld it first).  A face with a repeated index still connects its distinct ones.
// LABEL.  label[v] = the smallest vertex index of v's component; a vertex that no face names is its own label.  An exact function of
// the input, whatever the order in which the lanes run: the device returns the host build's numbers although it uses atomics.
// FOREST.  label is a parent array with label[v] <= v, equality for a root.  A union finds the two roots a, b by walking label, stops if
// a == b, and otherwise hooks the larger under the smaller by atomicCAS(&label[hi], hi, lo).  A parent is always smaller than its child,
// so no cycle can form and a walk from v reads at most v + 1 entries.  A CAS fails only when another lane has just given hi a parent,
// i.e. removed a root; at most V - 1 roots can be removed, so all retries of all lanes together are bounded by V, and no lane ever waits
// for another lane to act.  When all unions are done two vertices share a root exactly when a chain of faces connects them, and the root
// of a tree is its smallest member (every other member has a smaller parent): the flatten pass stores it.
// VISIBILITY.  Every read of label inside a walk or a retry loop is a relaxed atomic load at agent scope: a plain load may be hoisted out
// of the loop or served from a register or the CU's L1, and a lane that lost a CAS would never see the winner.  label carries no
// __restrict__.  The flatten pass writes label[v] while other lanes still walk through v: both the old parent and the root are ancestors,
// so a walk ends at the same root whichever it reads (relaxed atomic stores).
// GIVE-UP.  Every walk and every retry loop carries a step cap of V + 1, which the invariant never reaches on a forest; a lane that
// reaches it (a label array that is no forest: not this call's) ORs 1 into *status and returns.  Exercised on the host build only.
// Path shortening during the walk is not done (profiles/mesh_components.md has the timings it would have to beat).
#pragma once
#include "dsdf_winding.h"

namespace dsdf {

// the seam between the two builds, as DSDF_HD is for the arithmetic: the device's atomics, the serial host build's plain statements
#if defined(__HIP_DEVICE_COMPILE__)
#define DSDF_CC_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define DSDF_CC_STORE(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define DSDF_CC_CAS(p, expect, desired) atomicCAS((p), (expect), (desired))
#define DSDF_CC_GIVE_UP(status) atomicOr((status), 1)
#else
inline int32_t cc_host_cas(int32_t *p, int32_t expect, int32_t desired) { const int32_t old = *p; if (old == expect) *p = desired; return old; }
#define DSDF_CC_LOAD(p) (*(p))
#define DSDF_CC_STORE(p, v) (*(p) = (v))
#define DSDF_CC_CAS(p, expect, desired) cc_host_cas((p), (expect), (desired))
#define DSDF_CC_GIVE_UP(status) (*(status) |= 1)
#endif

// the root of v's tree, or -1 after cap reads without one (status set)
DSDF_HD int32_t cc_root(int32_t *label, int32_t v, int64_t cap, int32_t *status) {
    for (int64_t step = 0; step < cap; ++step) {
        const int32_t p = DSDF_CC_LOAD(label + v);
        if (p == v) return v;
        v = p;
    }
    DSDF_CC_GIVE_UP(status);
    return -1;
}

// a and b end up in one tree
DSDF_HD void cc_union(int32_t *label, int32_t a, int32_t b, int64_t cap, int32_t *status) {
    for (int64_t tries = 0; tries < cap; ++tries) {
        a = cc_root(label, a, cap, status);
        if (a < 0) return;
        b = cc_root(label, b, cap, status);
        if (b < 0) return;
        if (a == b) return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        if (DSDF_CC_CAS(label + hi, hi, lo) == hi) return;
        // hi got a parent from another lane meanwhile: go on from the two roots found, which are still members of the two trees
    }
    DSDF_CC_GIVE_UP(status);
}

// one face: (i0, i1) and (i1, i2)
DSDF_HD void cc_hook_face(const int32_t *faces, int64_t f, int32_t *label, int64_t cap, int32_t *status) {
    const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    cc_union(label, i0, i1, cap, status);
    cc_union(label, i1, i2, cap, status);
}

DSDF_HD void cc_flatten_vertex(int32_t *label, int32_t v, int64_t cap, int32_t *status) {
    const int32_t r = cc_root(label, v, cap, status);
    if (r >= 0) DSDF_CC_STORE(label + v, r);
}

// area = |(p1 - p0) x (p2 - p0)| / 2 and vol = p0 . (p1 x p2) / 6 of face f, every statement rounded on its own: the terms whose sums over
// a component are its area and (when it is closed) its signed volume
DSDF_HD void cc_face_measures(const float *vert, const int32_t *faces, int64_t f, float *area, float *vol) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float *a = vert + 3 * (size_t)faces[3 * f], *b = vert + 3 * (size_t)faces[3 * f + 1], *c = vert + 3 * (size_t)faces[3 * f + 2];
    const V3 p0 = mk(a[0], a[1], a[2]), p1 = mk(b[0], b[1], b[2]), p2 = mk(c[0], c[1], c[2]);
    const V3 N = cross_unfused(mk(p1.x - p0.x, p1.y - p0.y, p1.z - p0.z), mk(p2.x - p0.x, p2.y - p0.y, p2.z - p0.z));
    area[f] = 0.5f * sqrtf(dot_unfused(N, N));
    vol[f] = dot_unfused(p0, cross_unfused(p1, p2)) / 6.f;
}

}  // namespace dsdf

#if defined(__HIPCC__)
// =========================================================================================================================
// Kernels and entry points (fail / launch of dsdf_kernels.hip are in scope).
// =========================================================================================================================

__global__ __launch_bounds__(256) void k_cc_init(int32_t *label, int n_vertices) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n_vertices) label[v] = (int32_t)v;
}

// one lane per face: a coalesced read of its three indices, then walks through label that are as scattered as the mesh's numbering
__global__ __launch_bounds__(256) void k_cc_hook(const int32_t *__restrict__ faces, int64_t n_faces, int32_t *label, int64_t cap, int32_t *status) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f < n_faces) cc_hook_face(faces, f, label, cap, status);
}

__global__ __launch_bounds__(256) void k_cc_flatten(int32_t *label, int n_vertices, int64_t cap, int32_t *status) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n_vertices) cc_flatten_vertex(label, (int32_t)v, cap, status);
}

__global__ __launch_bounds__(256) void k_mesh_face_measures(const float *__restrict__ vert, const int32_t *__restrict__ faces, int64_t n_faces,
                                                            float *__restrict__ area, float *__restrict__ vol) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f < n_faces) cc_face_measures(vert, faces, f, area, vol);
}

extern "C" {

int dsdf_mesh_components(const int32_t *faces, int64_t n_faces, int n_vertices, int32_t *label, int32_t *status, void *stream) {
    if (n_vertices == 0) return DSDF_OK;
    if (n_vertices < 0 || n_faces < 0 || n_faces > (int64_t)0x7fffffff / 3 || !label || !status || (n_faces > 0 && !faces))
        return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_components: bad argument (null pointer, negative count, or 3 n_faces >= 2^31)");
    hipStream_t st = (hipStream_t)stream;
    const int64_t cap = (int64_t)n_vertices + 1;
    int rc;
    if ((rc = launch_lanes("k_cc_init", k_cc_init, n_vertices, st, label, n_vertices))) return rc;
    if (n_faces == 0) return DSDF_OK;
    if ((rc = launch_lanes("k_cc_hook", k_cc_hook, n_faces, st, faces, n_faces, label, cap, status))) return rc;
    return launch_lanes("k_cc_flatten", k_cc_flatten, n_vertices, st, label, n_vertices, cap, status);
}

int dsdf_mesh_face_measures(const float *vertices, const int32_t *faces, int64_t n_faces, float *area, float *vol, void *stream) {
    if (n_faces == 0) return DSDF_OK;
    if (!vertices || !faces || !area || !vol || n_faces < 0 || n_faces > (int64_t)0x7fffffff / 3)
        return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_face_measures: bad argument (null pointer, or 3 n_faces >= 2^31)");
    return launch_lanes("k_mesh_face_measures", k_mesh_face_measures, n_faces, (hipStream_t)stream, vertices, faces, n_faces, area, vol);
}

}  // extern "C"
#endif  // __HIPCC__
