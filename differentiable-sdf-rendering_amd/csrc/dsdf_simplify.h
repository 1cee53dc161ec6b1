// dsdf_simplify.h -- mesh simplification by vertex clustering with quadric error metrics (Lindstrom 2000): all vertices of an indexed
// mesh that fall into one cell of a regular grid become ONE vertex, placed where the summed squared distance to the planes of the cell's
// triangles is smallest (a flat region stays flat, a crease or a corner keeps its position); triangles that lose a corner disappear.
// Every cell is independent of every other -- which is why this variant, and not sequential edge collapse, runs on a GPU.
//
// Two parts, like dsdf_winding.h (whose cross_unfused it shares): host/device inline arithmetic that any C++ compiler builds -- the
// host-side tests run exactly these statements -- and, under __HIPCC__, the kernels and the C-ABI entry points (dsdf_kernels.hip includes
// this file after dsdf_winding.h).  No atomics, no allocation, no synchronisation: the sort of the corner keys and the scans between the
// launches are the caller's (plumbing, as the sort in front of dsdf_mesh_bvh_build and the scans of dsdf_iso_*).
//
// CELLS.  A box lo / hi cut into cx x cy x cz cells, cx cy cz < 2^31.  Per axis i = clamp(floor((v - lo) inv), 0, c - 1) with
// inv = c / (hi - lo) computed ONCE on the host in float; key = (iz cy + iy) cx + ix.  A vertex outside the box lands in the border cell.
// CORNER RECORDS.  Corner 3 f + k of face f carries the key of its vertex.  The caller sorts the 3 F keys (stable), which yields the
// U OCCUPIED cells (a cell with at least one face corner; a vertex no face uses plays no part) as segments of the sorted corner ids.
// A face SURVIVES when its three cells differ; a cell is USED when a surviving face has a corner in it.  Output vertices = the used
// cells in ascending key; output faces = the survivors in input order, winding kept.  Duplicate faces, and the opposite pairs a
// collapsing thin sheet leaves, are kept as they are; non-manifold edges can appear.
// REPRESENTATIVE of a used cell: ONE lane walks the cell's segment in sorted order and recomputes the quadric of every record from its
// face, in coordinates relative to the cell's centre (what keeps fp32 usable): N = (p1 - p0) x (p2 - p0); |N| = 0 adds no quadric;
// otherwise n = N / |N|, a = |N| / 2, d = -n . (p0 - centre), A += a n n^T, b += a d n, area += a, Nsum += N / 2.  Every record also adds
// its own corner's position to the mean m (and its colour to the colour mean).  x = argmin x^T A x + 2 b^T x + lambda |x - m|^2 with
// lambda = reg area: the SPD system (A + lambda I) x = lambda m - b, solved by Cholesky -- only + - x / sqrtf, each rounded on its own
// (no contraction) and correctly rounded in both builds, so the device returns the host build's BITS.  The regulariser bounds the
// condition number by about 1 / reg: a flat patch (A of rank 1) gets a well-defined vertex on its plane next to the mean.  area = 0 (or
// a failed factorisation: non-finite input): x = m.  x is clamped into the cell's box [-h, h] around the centre.
#pragma once
#include "dsdf_winding.h"

namespace dsdf {

#ifndef DSDF_SIMPLIFY_REG
#define DSDF_SIMPLIFY_REG 1e-3f   /* (include/dsdf.h has it for callers) */
#endif

struct SimplifyGrid { float lo[3], inv[3], size[3]; int c[3]; };

// The grid of a call from its arguments, on the host: nullptr, or what is wrong with them.
inline const char *simplify_grid(const float *lo, const float *hi, int cx, int cy, int cz, SimplifyGrid &G) {
    if (!lo || !hi) return "lo / hi is null";
    if (cx < 1 || cy < 1 || cz < 1) return "cell counts must be >= 1";
    if ((int64_t)cx * cy >= ((int64_t)1 << 31) || (int64_t)cx * cy * cz >= ((int64_t)1 << 31)) return "cx * cy * cz must stay below 2^31";
    const int c[3] = {cx, cy, cz};
    for (int a = 0; a < 3; ++a) {
        const float ext = hi[a] - lo[a];
        if (!(ext > 0.f && ext < INFINITY)) return "need lo < hi (finite) on every axis";
        G.lo[a] = lo[a]; G.c[a] = c[a];
        G.inv[a] = (float)c[a] / ext;
        G.size[a] = ext / (float)c[a];
    }
    return nullptr;
}

DSDF_HD int simplify_axis(float v, float lo, float inv, int c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float t = floorf((v - lo) * inv);
    const int i = t >= 0.f ? (t < (float)c ? (int)t : c - 1) : 0;        // (NaN: cell 0)
    return i < c ? i : c - 1;                                             // ((float)c may have rounded up)
}

DSDF_HD int simplify_key(const SimplifyGrid &G, const float *v) {
    const int ix = simplify_axis(v[0], G.lo[0], G.inv[0], G.c[0]), iy = simplify_axis(v[1], G.lo[1], G.inv[1], G.c[1]);
    const int iz = simplify_axis(v[2], G.lo[2], G.inv[2], G.c[2]);
    return (iz * G.c[1] + iy) * G.c[0] + ix;
}

// the rank of `key` among the n ascending, distinct keys of the occupied cells (the caller looks up keys that are present)
DSDF_HD int simplify_rank(const int32_t *cell_keys, int n, int key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cell_keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one face: the ranks of its three cells; it survives when they differ, and a survivor marks its cells as used (several threads storing
// the same 1 is fine)
DSDF_HD void simplify_mark_face(const int32_t *keys, int64_t f, const int32_t *cell_keys, int n_cells, int32_t *rank, int32_t *keep, int32_t *used) {
    const int r0 = simplify_rank(cell_keys, n_cells, keys[3 * f]), r1 = simplify_rank(cell_keys, n_cells, keys[3 * f + 1]);
    const int r2 = simplify_rank(cell_keys, n_cells, keys[3 * f + 2]);
    rank[3 * f] = r0; rank[3 * f + 1] = r1; rank[3 * f + 2] = r2;
    const bool alive = r0 != r1 && r1 != r2 && r2 != r0 && r0 < n_cells && r1 < n_cells && r2 < n_cells;      // (a key beyond the last cell: not this call's keys)
    keep[f] = alive ? 1 : 0;
    if (alive) { used[r0] = 1; used[r1] = 1; used[r2] = 1; }
}

// the representative of one cell from the records [begin, end) of the sorted corner ids: position (3 floats), normal and colour unless NULL
DSDF_HD void simplify_cell(const SimplifyGrid &G, float reg, const float *vert, const int32_t *faces, const float *colors, const int32_t *corner,
                           int begin, int end, int key, float *pos, float *nrm, float *col) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int ix = key % G.c[0], iy = (key / G.c[0]) % G.c[1], iz = key / (G.c[0] * G.c[1]);
    const V3 ctr = mk(G.lo[0] + ((float)ix + 0.5f) * G.size[0], G.lo[1] + ((float)iy + 0.5f) * G.size[1], G.lo[2] + ((float)iz + 0.5f) * G.size[2]);
    const V3 h = mk(0.5f * G.size[0], 0.5f * G.size[1], 0.5f * G.size[2]);
    float a00 = 0.f, a01 = 0.f, a02 = 0.f, a11 = 0.f, a12 = 0.f, a22 = 0.f, area = 0.f;
    V3 b = mk(0.f, 0.f, 0.f), ns = mk(0.f, 0.f, 0.f), ms = mk(0.f, 0.f, 0.f), cs = mk(0.f, 0.f, 0.f);
    for (int s = begin; s < end; ++s) {
        const int e = corner[s], f = e / 3;
        const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
        const int own = e - 3 * f == 0 ? i0 : (e - 3 * f == 1 ? i1 : i2);
        const float *p0 = vert + 3 * (size_t)i0, *p1 = vert + 3 * (size_t)i1, *p2 = vert + 3 * (size_t)i2, *po = vert + 3 * (size_t)own;
        const V3 N = cross_unfused(mk(p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]), mk(p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]));
        const float len = sqrtf(dot_unfused(N, N));
        if (len > 0.f && len < INFINITY) {
            const V3 n = mk(N.x / len, N.y / len, N.z / len);
            const float a = 0.5f * len;
            const float d = -dot_unfused(n, mk(p0[0] - ctr.x, p0[1] - ctr.y, p0[2] - ctr.z));
            const V3 an = mk(a * n.x, a * n.y, a * n.z);
            a00 = a00 + an.x * n.x; a01 = a01 + an.x * n.y; a02 = a02 + an.x * n.z;
            a11 = a11 + an.y * n.y; a12 = a12 + an.y * n.z; a22 = a22 + an.z * n.z;
            b = mk(b.x + d * an.x, b.y + d * an.y, b.z + d * an.z);
            area = area + a;
            ns = mk(ns.x + 0.5f * N.x, ns.y + 0.5f * N.y, ns.z + 0.5f * N.z);
        }
        ms = mk(ms.x + (po[0] - ctr.x), ms.y + (po[1] - ctr.y), ms.z + (po[2] - ctr.z));
        if (col) { const float *c = colors + 3 * (size_t)own; cs = mk(cs.x + c[0], cs.y + c[1], cs.z + c[2]); }
    }
    const float cnt = (float)(end - begin);
    const V3 m = mk(ms.x / cnt, ms.y / cnt, ms.z / cnt);
    V3 x = m;
    if (area > 0.f) {
        // (A + lambda I) x = lambda m - b by Cholesky, L L^T: forward, then backward substitution
        const float lam = reg * area;
        const float m00 = a00 + lam, m11 = a11 + lam, m22 = a22 + lam;
        const V3 r = mk(lam * m.x - b.x, lam * m.y - b.y, lam * m.z - b.z);
        const float l00 = sqrtf(m00), l10 = a01 / l00, l20 = a02 / l00;
        const float q11 = m11 - l10 * l10, l11 = sqrtf(q11), l21 = (a12 - l20 * l10) / l11;
        const float q22 = m22 - l20 * l20 - l21 * l21, l22 = sqrtf(q22);
        if (m00 > 0.f && q11 > 0.f && q22 > 0.f) {
            const float y0 = r.x / l00, y1 = (r.y - l10 * y0) / l11, y2 = (r.z - l20 * y0 - l21 * y1) / l22;
            const float x2 = y2 / l22, x1 = (y1 - l21 * x2) / l11, x0 = (y0 - l10 * x1 - l20 * x2) / l00;
            if (x0 - x0 == 0.f && x1 - x1 == 0.f && x2 - x2 == 0.f) x = mk(x0, x1, x2);       // (finite)
        }
    }
    x.x = x.x > -h.x ? x.x : -h.x; x.x = x.x < h.x ? x.x : h.x;            // into the cell's box (NaN: the lower face)
    x.y = x.y > -h.y ? x.y : -h.y; x.y = x.y < h.y ? x.y : h.y;
    x.z = x.z > -h.z ? x.z : -h.z; x.z = x.z < h.z ? x.z : h.z;
    pos[0] = ctr.x + x.x; pos[1] = ctr.y + x.y; pos[2] = ctr.z + x.z;
    if (nrm) {
        const float len = sqrtf(dot_unfused(ns, ns));
        const bool ok = len > 0.f && len < INFINITY;
        nrm[0] = ok ? ns.x / len : 0.f; nrm[1] = ok ? ns.y / len : 0.f; nrm[2] = ok ? ns.z / len : 0.f;
    }
    if (col) { col[0] = cs.x / cnt; col[1] = cs.y / cnt; col[2] = cs.z / cnt; }
}

}  // namespace dsdf

#if defined(__HIPCC__)
// =========================================================================================================================
// Kernels and entry points (fail / launch of dsdf_kernels.hip are in scope).
// =========================================================================================================================

// one lane per face corner: coalesced reads of the face indices, a scattered gather of one vertex each
__global__ __launch_bounds__(256) void k_simplify_keys(SimplifyGrid G, const float *__restrict__ vert, const int32_t *__restrict__ faces, int64_t n_corners,
                                                       int32_t *__restrict__ keys) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n_corners) keys[e] = simplify_key(G, vert + 3 * (size_t)faces[e]);
}

// one lane per face: three binary searches in the occupied keys (log2 U steps each; their first steps hit the same few lines for every lane)
__global__ __launch_bounds__(256) void k_simplify_mark(const int32_t *__restrict__ keys, int64_t n_faces, const int32_t *__restrict__ cell_keys, int n_cells,
                                                       int32_t *__restrict__ rank, int32_t *__restrict__ keep, int32_t *used) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f < n_faces) simplify_mark_face(keys, f, cell_keys, n_cells, rank, keep, used);
}

__global__ __launch_bounds__(256) void k_simplify_faces(const int32_t *__restrict__ rank, const int32_t *__restrict__ keep, const int32_t *__restrict__ face_offset,
                                                        const int32_t *__restrict__ vertex_id, int64_t n_faces, int32_t *__restrict__ faces_out) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_faces || !keep[f]) return;
    int32_t *o = faces_out + 3 * (size_t)face_offset[f];
    o[0] = vertex_id[rank[3 * f]]; o[1] = vertex_id[rank[3 * f + 1]]; o[2] = vertex_id[rank[3 * f + 2]];
}

// One lane per occupied cell.  The segments of neighbouring cells are adjacent in the sorted corner ids (consecutive lanes read
// consecutive lines of them); the face and vertex gathers behind them are scattered, as in any indexed mesh.  Blocks of 64: the lanes of
// a wave run as long as its longest segment, and small blocks spread the long ones over the chip.
__global__ __launch_bounds__(64) void k_simplify_cells(SimplifyGrid G, float reg, const float *__restrict__ vert, const int32_t *__restrict__ faces,
                                                       const float *__restrict__ colors, const int32_t *__restrict__ corner, const int32_t *__restrict__ cell_keys,
                                                       const int32_t *__restrict__ cell_start, int n_cells, const int32_t *__restrict__ used,
                                                       const int32_t *__restrict__ vertex_id, float *__restrict__ pos, float *__restrict__ nrm, float *__restrict__ col) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_cells || !used[r]) return;
    const size_t o = 3 * (size_t)vertex_id[r];
    simplify_cell(G, reg, vert, faces, colors, corner, cell_start[r], cell_start[r + 1], cell_keys[r], pos + o, nrm ? nrm + o : nullptr,
                  col ? col + o : nullptr);
}

extern "C" {

int dsdf_simplify_keys(const float *vertices, const int32_t *faces, int64_t n_faces, const float *lo, const float *hi, int cx, int cy, int cz,
                       int32_t *keys_out, void *stream) {
    char msg[160];
    SimplifyGrid G;
    if (const char *why = simplify_grid(lo, hi, cx, cy, cz, G)) { snprintf(msg, sizeof(msg), "dsdf_simplify_keys: %s", why); return fail(DSDF_ERR_INVALID_ARG, msg); }
    if (n_faces == 0) return DSDF_OK;
    if (!vertices || !faces || !keys_out || n_faces < 0 || n_faces > (int64_t)0x7fffffff / 3)
        return fail(DSDF_ERR_INVALID_ARG, "dsdf_simplify_keys: bad argument (null pointer, or 3 n_faces >= 2^31)");
    const int64_t n = 3 * n_faces;
    return launch_lanes("k_simplify_keys", k_simplify_keys, n, (hipStream_t)stream, G, vertices, faces, n, keys_out);
}

int dsdf_simplify_mark(const int32_t *keys, int64_t n_faces, const int32_t *cell_keys, int n_cells, int32_t *rank_out, int32_t *keep_out,
                       int32_t *used, void *stream) {
    if (n_faces == 0) return DSDF_OK;
    if (!keys || !cell_keys || !rank_out || !keep_out || !used || n_faces < 0 || n_faces > (int64_t)0x7fffffff / 3 || n_cells < 1)
        return fail(DSDF_ERR_INVALID_ARG, "dsdf_simplify_mark: bad argument");
    return launch_lanes("k_simplify_mark", k_simplify_mark, n_faces, (hipStream_t)stream, keys, n_faces, cell_keys,
                  n_cells, rank_out, keep_out, used);
}

int dsdf_simplify_emit(const float *vertices, const int32_t *faces, int64_t n_faces, const float *colors, const float *lo, const float *hi, int cx,
                       int cy, int cz, float reg, const int32_t *corner, const int32_t *cell_keys, const int32_t *cell_start, int n_cells,
                       const int32_t *rank, const int32_t *keep, const int32_t *face_offset, const int32_t *used, const int32_t *vertex_id,
                       int32_t *faces_out, float *positions_out, float *normals_out, float *colors_out, void *stream) {
    char msg[160];
    SimplifyGrid G;
    if (const char *why = simplify_grid(lo, hi, cx, cy, cz, G)) { snprintf(msg, sizeof(msg), "dsdf_simplify_emit: %s", why); return fail(DSDF_ERR_INVALID_ARG, msg); }
    if (!(reg > 0.f && reg < INFINITY)) return fail(DSDF_ERR_INVALID_ARG, "dsdf_simplify_emit: reg must be > 0");
    if (n_faces == 0) return DSDF_OK;
    if (!vertices || !faces || !corner || !cell_keys || !cell_start || !rank || !keep || !face_offset || !used || !vertex_id || !faces_out ||
        !positions_out || n_faces < 0 || n_faces > (int64_t)0x7fffffff / 3 || n_cells < 1 || (colors_out && !colors))
        return fail(DSDF_ERR_INVALID_ARG, "dsdf_simplify_emit: bad argument");
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = launch_lanes("k_simplify_faces", k_simplify_faces, n_faces, st, rank, keep, face_offset, vertex_id, n_faces,
                     faces_out))) return rc;
    return launch("k_simplify_cells", k_simplify_cells, dim3((unsigned)((n_cells + 63) / 64)), dim3(64), st, G, reg, vertices, faces, colors, corner, cell_keys,
                  cell_start, n_cells, used, vertex_id, positions_out, normals_out, colors_out);
}

}  // extern "C"
#endif  // __HIPCC__
