// dsdf_iso.h -- triangle mesh of the RENDERED surface: the level set {f = iso} of the tricubic B-spline lookup f (eval_cubic), not of the
// voxel values (the B-spline does not interpolate its coefficients).  Marching tetrahedra on a lattice of nx x ny x nz cells over the
// unit cube of the grid, in the cube's own frame (`sdf.p` and a to_world play no part; python/dsdf maps the result out).
//
//   k_iso_sample   values[node] = f(node)                                     one thread per node
//   k_iso_mark     cross[node] (bit t: the edge of type t crosses), n_vert[node], n_tri[node]      one thread per node
//   (two exclusive scans of the counts: the caller's, like the sort in front of dsdf_mesh_bvh_build)
//   k_iso_emit     vert_edge[v] = 8 node + type, faces[f] = three vertex ids   one thread per node, nodes without a crossing edge leave
//   k_iso_refine   positions / normals                                         one thread per VERTEX of the compacted list
//
// TOPOLOGY IS A FUNCTION OF THE BUFFER `values` ALONE: a node is inside iff values[node] < iso (strict), and mark / emit / the first
// bracket of refine read the sign there and nowhere else, so a caller (or a test oracle) that is handed the buffer reproduces every
// count and index exactly -- a lookup that comes out 1e-6 on the other side of iso elsewhere cannot tear the mesh.
//
// Lattice: nodes (i/nx, j/ny, k/nz), node index (k (ny + 1) + j)(nx + 1) + i.  A node OWNS the up to seven edges towards its upper
// neighbours, type 0 +x, 1 +y, 2 +z, 3 +x+y, 4 +x+z, 5 +y+z, 6 +x+y+z (an edge exists when its far node does); an edge whose ends lie on
// different sides carries exactly one vertex; vertices are ordered by owning node, then type.  A cell (lower corner c) is cut into the
// six Kuhn tetrahedra around the diagonal c .. c + (1,1,1): one per axis order (a, b, d), corners v0 = c, v1 = c + e_a, v2 = c + e_a + e_b,
// v3 = c + (1,1,1), numbered 0..5 for xyz, xzy, yxz, yzx, zxy, zyx.  The cut is the same in every cell, so neighbours agree on the
// diagonals of their shared faces, and every tetrahedron edge is one of the seven edge types of its lower end.  Per tetrahedron, with I
// the inside and O the outside corners (ascending) and e(p, q) the vertex on edge vp vq:
//   |I| = 1, I = {a}:               e(a,O0) e(a,O1) e(a,O2)
//   |I| = 3, O = {d}:               e(I0,d) e(I1,d) e(I2,d)
//   |I| = 2, I = {a,b}, O = {c,d}:  q0 q1 q2 and q0 q2 q3 of the quad q = e(a,c) e(a,d) e(b,d) e(b,c)
// and the last two vertices of a triangle are swapped where (B - A) x (C - A) would otherwise point from the outside corners to the inside
// ones.  Whether it would depends on the case and on the handedness of the tetrahedron only (the sign of a determinant of corner
// differences; where the vertices sit on their edges scales it by positive factors): iso_swap below.  Faces are ordered by cell, then
// tetrahedron, then as listed.  16 sign cases and at most 2 triangles per tetrahedron: no 256-entry table.
//
// A surface that leaves the cube is NOT capped: the mesh is open along the lattice border there.
//
// k_iso_mark reads the 8 corner values of a node's cell straight from global memory and leaves the 8-fold reuse to the caches: a wave
// covers 64 x-consecutive nodes, so its 8 reads are 4 row segments of 65 floats, each fetched twice back to back from the same lines
// (L1), and the rows of the next y / z come from the L2, which holds two node planes of any lattice the 2^27 limit admits.  The kernel
// moves 4 B in and 9 B out per node from HBM either way; an LDS tile would add a barrier and halo loads and remove no HBM traffic.
#pragma once
#include "dsdf_math.h"

namespace dsdf {

#define DSDF_ISO_MAX_NODES (1ll << 27)   /* 8 node + type and 12 nodes (the most triangles) fit an int32 */

struct IsoLattice {
    int nx, ny, nz;
    int sx, sxy;          // nodes per row, per plane
    float fnx, fny, fnz;
};

DSDF_HD IsoLattice iso_lattice(int nx, int ny, int nz) {
    IsoLattice L;
    L.nx = nx; L.ny = ny; L.nz = nz;
    L.sx = nx + 1; L.sxy = (nx + 1) * (ny + 1);
    L.fnx = (float)nx; L.fny = (float)ny; L.fnz = (float)nz;
    return L;
}
DSDF_HD int64_t iso_node_count(int nx, int ny, int nz) { return (int64_t)(nx + 1) * (int64_t)(ny + 1) * (int64_t)(nz + 1); }
DSDF_HD void iso_node_ijk(const IsoLattice &L, int node, int &i, int &j, int &k) {
    k = node / L.sxy;
    const int r = node - k * L.sxy;
    j = r / L.sx;
    i = r - j * L.sx;
}
DSDF_HD V3 iso_node_pos(const IsoLattice &L, int i, int j, int k) { return mk((float)i / L.fnx, (float)j / L.fny, (float)k / L.fnz); }

// A cell corner or an edge direction as a code: bit 0 +x, bit 1 +y, bit 2 +z.  Edge type t has the code {1, 2, 4, 3, 5, 6, 7}[t].
DSDF_HD int iso_type_code(int t) { return (0x7653421 >> (4 * t)) & 7; }
DSDF_HD int iso_code_type(int c) { return (0x65423100 >> (4 * c)) & 7; }          // (code 0 is no edge)
DSDF_HD int iso_code_offset(const IsoLattice &L, int c) { return (c & 1) + ((c >> 1) & 1) * L.sx + ((c >> 2) & 1) * L.sxy; }
// corners v1, v2 of tetrahedron 0..5 as codes (v0 = 0, v3 = 7): xyz 1 3, xzy 1 5, yxz 2 3, yzx 2 6, zxy 4 5, zyx 4 6
DSDF_HD int iso_tet_corner(int tet, int p) {
    return p == 0 ? 0 : p == 3 ? 7 : p == 1 ? ((0x442211 >> (4 * tet)) & 7) : ((0x656353 >> (4 * tet)) & 7);
}
// 1: swap the last two vertices of the triangles of this (tetrahedron, case).  Tetrahedra 0, 3, 4 (xyz, yzx, zxy: even orders) are
// right-handed, det[v1 - v0, v2 - v0, v3 - v0] = +1, the others left-handed; bit `case` of 0x4d24 is the answer for a right-handed one
// (case = bit p set when corner vp is inside), derived from the rule in the header and checked against it by tests/test_iso_host.py.
DSDF_HD int iso_swap(int tet, int mask) { return ((0x4d24 >> mask) ^ (0x26 >> tet)) & 1; }
DSDF_HD int iso_popc(unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}
// triangles of a tetrahedron case: 0, 1 or 2
DSDF_HD int iso_case_tris(int mask) { const int c = iso_popc((unsigned)mask); return (c == 0 || c == 4) ? 0 : (c == 2 ? 2 : 1); }

// Inside bits of the 8 corners of the cell whose lower corner is `node` (bit = corner code); corners outside the lattice read as the
// node itself (no crossing).  `have`: the codes of the axes along which an upper neighbour exists.
DSDF_HD int iso_cube_mask(const IsoLattice &L, const float *values, float iso, int node, int have) {
    int m = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int cc = c & have;
        m |= (values[node + iso_code_offset(L, cc)] < iso ? 1 : 0) << c;
    }
    return m;
}
DSDF_HD int iso_have(const IsoLattice &L, int i, int j, int k) { return (i < L.nx ? 1 : 0) | (j < L.ny ? 2 : 0) | (k < L.nz ? 4 : 0); }
DSDF_HD int iso_tet_mask(int tet, int cube) {
    return (cube & 1) | (((cube >> iso_tet_corner(tet, 1)) & 1) << 1) | (((cube >> iso_tet_corner(tet, 2)) & 1) << 2) | (((cube >> 7) & 1) << 3);
}

// ---- per-node statements -------------------------------------------------------------------------------------------------------
DSDF_HD void iso_sample_node(const GridView &G, const IsoLattice &L, int node, float *values) {
    int i, j, k;
    iso_node_ijk(L, node, i, j, k);
    float v; V3 g; float H[6];
    eval_cubic_local<0>(G, iso_node_pos(L, i, j, k), v, g, H);
    values[node] = v;
}

DSDF_HD void iso_mark_node(const IsoLattice &L, const float *values, float iso, int node, uint8_t *cross, int32_t *n_vert, int32_t *n_tri) {
    int i, j, k;
    iso_node_ijk(L, node, i, j, k);
    const int have = iso_have(L, i, j, k);
    const int cube = iso_cube_mask(L, values, iso, node, have);
    const int in0 = cube & 1;
    int cr = 0;
#pragma unroll
    for (int t = 0; t < 7; ++t) {
        const int c = iso_type_code(t);
        if ((c & have) == c && ((cube >> c) & 1) != in0) cr |= 1 << t;
    }
    int nt = 0;
    if (have == 7) {
#pragma unroll
        for (int tet = 0; tet < 6; ++tet) nt += iso_case_tris(iso_tet_mask(tet, cube));
    }
    cross[node] = (uint8_t)cr;
    n_vert[node] = iso_popc((unsigned)cr);
    n_tri[node] = nt;
}

// the id of the vertex on the edge between corners (codes) cp < cq of the cell at `node`
DSDF_HD int32_t iso_vertex_id(const IsoLattice &L, const uint8_t *cross, const int32_t *vert_offset, int node, int cp, int cq) {
    const int m = node + iso_code_offset(L, cp);
    const int t = iso_code_type(cq ^ cp);
    return vert_offset[m] + iso_popc((unsigned)cross[m] & ((1u << t) - 1u));
}

DSDF_HD void iso_emit_node(const IsoLattice &L, const float *values, float iso, const uint8_t *cross, const int32_t *vert_offset,
                           const int32_t *tri_offset, int node, int32_t *vert_edge, int32_t *faces) {
    const int cr = cross[node];
    if (cr == 0) return;                          // no crossing edge: no vertex, and a cell with triangles has one at its lower corner
    int v = vert_offset[node];
    for (int t = 0; t < 7; ++t)
        if ((cr >> t) & 1) vert_edge[v++] = 8 * node + t;
    int i, j, k;
    iso_node_ijk(L, node, i, j, k);
    if (iso_have(L, i, j, k) != 7) return;
    const int cube = iso_cube_mask(L, values, iso, node, 7);
    int32_t *f = faces + 3 * (size_t)tri_offset[node];
    for (int tet = 0; tet < 6; ++tet) {
        const int mask = iso_tet_mask(tet, cube);
        const int ntri = iso_case_tris(mask);
        if (ntri == 0) continue;
        int in[4], out[4], ni = 0, no = 0;
        for (int p = 0; p < 4; ++p) { if ((mask >> p) & 1) in[ni++] = p; else out[no++] = p; }
        // the (up to four) vertices in the order of the header: pairs of tetrahedron corners
        int ep[4], eq[4], nq;
        if (ni == 1) { nq = 3; for (int r = 0; r < 3; ++r) { ep[r] = in[0]; eq[r] = out[r]; } }
        else if (ni == 3) { nq = 3; for (int r = 0; r < 3; ++r) { ep[r] = in[r]; eq[r] = out[0]; } }
        else { nq = 4; ep[0] = in[0]; eq[0] = out[0]; ep[1] = in[0]; eq[1] = out[1]; ep[2] = in[1]; eq[2] = out[1]; ep[3] = in[1]; eq[3] = out[0]; }
        int32_t id[4];
        for (int r = 0; r < nq; ++r) {
            const int a = ep[r] < eq[r] ? ep[r] : eq[r], b = ep[r] < eq[r] ? eq[r] : ep[r];
            id[r] = iso_vertex_id(L, cross, vert_offset, node, iso_tet_corner(tet, a), iso_tet_corner(tet, b));
        }
        const int sw = iso_swap(tet, mask);
        f[0] = id[0]; f[1] = sw ? id[2] : id[1]; f[2] = sw ? id[1] : id[2];
        f += 3;
        if (ntri == 2) {
            f[0] = id[0]; f[1] = sw ? id[3] : id[2]; f[2] = sw ? id[2] : id[3];
            f += 3;
        }
    }
}

// ---- per-vertex statement: the root of f on the lattice edge by `steps` bisection steps from the signs of `values`; the position is
// a + ((s0 + s1) / 2)(b - a); the normal the normalised gradient of f there (a zero gradient: the edge direction towards the outside end)
DSDF_HD void iso_refine_vertex(const GridView &G, const IsoLattice &L, const float *values, float iso, const int32_t *vert_edge, int64_t v,
                               int steps, float *positions, float *normals) {
    const int ve = vert_edge[v];
    const int node = ve >> 3, code = iso_type_code(ve & 7);
    int i, j, k;
    iso_node_ijk(L, node, i, j, k);
    const V3 a = iso_node_pos(L, i, j, k);
    const V3 d = iso_node_pos(L, i + (code & 1), j + ((code >> 1) & 1), k + ((code >> 2) & 1)) - a;
    const bool inside_a = values[node] < iso;
    float s0 = 0.f, s1 = 1.f;
    for (int it = 0; it < steps; ++it) {
        const float sm = 0.5f * (s0 + s1);
        float fv; V3 g; float H[6];
        eval_cubic_local<0>(G, fma3(sm, d, a), fv, g, H);
        if ((fv < iso) == inside_a) s0 = sm; else s1 = sm;
    }
    const V3 p = fma3(0.5f * (s0 + s1), d, a);
    positions[3 * v] = p.x; positions[3 * v + 1] = p.y; positions[3 * v + 2] = p.z;
    if (normals) {
        float fv; V3 g; float H[6];
        eval_cubic_local<1>(G, p, fv, g, H);
        float n2 = dot(g, g);
        if (!(n2 > 0.f)) { g = inside_a ? d : -d; n2 = dot(g, g); }
        const float r = 1.f / sqrtf(n2);
        normals[3 * v] = g.x * r; normals[3 * v + 1] = g.y * r; normals[3 * v + 2] = g.z * r;
    }
}

// ---- colours for the vertices: the value of a (Z,Y,X,channels) volume at a point, channels 1 or 3 ----------------------------------
// What the direct integrator reads there: eval_trilinear / eval_trilinear1 (dsdf_math.h) with the gradient dropped.
DSDF_HD void volume_sample_point(const AlbedoView &A, int channels, const float *points, int64_t i, float *out) {
    const V3 p = mk(points[3 * i], points[3 * i + 1], points[3 * i + 2]);
    if (channels == 3) {
        float val[3]; V3 grad[3];
        eval_trilinear(A, p, val, grad);
        out[3 * i] = val[0]; out[3 * i + 1] = val[1]; out[3 * i + 2] = val[2];
    } else {
        float val; V3 grad;
        eval_trilinear1(A, p, val, grad);
        out[i] = val;
    }
}

}  // namespace dsdf

#if defined(__HIPCC__)
using namespace dsdf;

__global__ __launch_bounds__(256) void k_volume_sample(AlbedoView A, int channels, const float *__restrict__ points, int64_t n, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) volume_sample_point(A, channels, points, i, out);
}

__global__ __launch_bounds__(256) void k_iso_sample(GridView G, IsoLattice L, int n_nodes, float *__restrict__ values) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node < n_nodes) iso_sample_node(G, L, node, values);
}

__global__ __launch_bounds__(256) void k_iso_mark(IsoLattice L, int n_nodes, const float *__restrict__ values, float iso, uint8_t *__restrict__ cross,
                                                  int32_t *__restrict__ n_vert, int32_t *__restrict__ n_tri) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node < n_nodes) iso_mark_node(L, values, iso, node, cross, n_vert, n_tri);
}

__global__ __launch_bounds__(256) void k_iso_emit(IsoLattice L, int n_nodes, const float *__restrict__ values, float iso, const uint8_t *__restrict__ cross,
                                                  const int32_t *__restrict__ vert_offset, const int32_t *__restrict__ tri_offset,
                                                  int32_t *__restrict__ vert_edge, int32_t *__restrict__ faces) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node < n_nodes) iso_emit_node(L, values, iso, cross, vert_offset, tri_offset, node, vert_edge, faces);
}

__global__ __launch_bounds__(256) void k_iso_refine(GridView G, IsoLattice L, const float *__restrict__ values, float iso,
                                                    const int32_t *__restrict__ vert_edge, int64_t n_vert, int steps, float *__restrict__ positions,
                                                    float *__restrict__ normals) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n_vert) iso_refine_vertex(G, L, values, iso, vert_edge, v, steps, positions, normals);
}

// the shared checks of the four entry points; 0 = fine
static int iso_check_lattice(const char *who, int nx, int ny, int nz) {
    char msg[160];
    if (nx < 1 || ny < 1 || nz < 1) {
        snprintf(msg, sizeof(msg), "%s: the lattice needs at least one cell per axis", who);
        return fail(DSDF_ERR_INVALID_ARG, msg);
    }
    if (iso_node_count(nx, ny, nz) > DSDF_ISO_MAX_NODES) {
        snprintf(msg, sizeof(msg), "%s: more than 2^27 lattice nodes", who);
        return fail(DSDF_ERR_INVALID_ARG, msg);
    }
    return DSDF_OK;
}

static GridView iso_view(const float *padded, int rx, int ry, int rz) {
    dsdf_params prm;
    dsdf_default_params(&prm);                     // (sdf.p = 0; the lookups of this header take cube coordinates and read no parameter)
    return device_view(padded, rx, ry, rz, prm);
}

extern "C" {

int dsdf_iso_sample(const float *padded, int rx, int ry, int rz, int nx, int ny, int nz, float *values, void *stream) {
    if (!padded || !values) return fail(DSDF_ERR_INVALID_ARG, "dsdf_iso_sample: null pointer argument");
    if (rx < 1 || ry < 1 || rz < 1) return fail(DSDF_ERR_INVALID_ARG, "dsdf_iso_sample: bad grid size");
    if (int rc = iso_check_lattice("dsdf_iso_sample", nx, ny, nz)) return rc;
    const int n = (int)iso_node_count(nx, ny, nz);
    return launch_lanes("k_iso_sample", k_iso_sample, n, (hipStream_t)stream, iso_view(padded, rx, ry, rz),
                  iso_lattice(nx, ny, nz), n, values);
}

int dsdf_iso_mark(const float *values, int nx, int ny, int nz, float iso, uint8_t *cross, int32_t *n_vert, int32_t *n_tri, void *stream) {
    if (!values || !cross || !n_vert || !n_tri) return fail(DSDF_ERR_INVALID_ARG, "dsdf_iso_mark: null pointer argument");
    if (int rc = iso_check_lattice("dsdf_iso_mark", nx, ny, nz)) return rc;
    const int n = (int)iso_node_count(nx, ny, nz);
    return launch_lanes("k_iso_mark", k_iso_mark, n, (hipStream_t)stream, iso_lattice(nx, ny, nz), n, values, iso,
                  cross, n_vert, n_tri);
}

int dsdf_iso_emit(const float *values, int nx, int ny, int nz, float iso, const uint8_t *cross, const int32_t *vert_offset,
                  const int32_t *tri_offset, int32_t *vert_edge, int32_t *faces, void *stream) {
    // (vert_edge / faces may be null when the caller's totals are zero: nothing is written then)
    if (!values || !cross || !vert_offset || !tri_offset) return fail(DSDF_ERR_INVALID_ARG, "dsdf_iso_emit: null pointer argument");
    if (int rc = iso_check_lattice("dsdf_iso_emit", nx, ny, nz)) return rc;
    if (!vert_edge) return DSDF_OK;                // no vertex, hence no face
    const int n = (int)iso_node_count(nx, ny, nz);
    return launch_lanes("k_iso_emit", k_iso_emit, n, (hipStream_t)stream, iso_lattice(nx, ny, nz), n, values, iso,
                  cross, vert_offset, tri_offset, vert_edge, faces);
}

int dsdf_iso_refine(const float *padded, int rx, int ry, int rz, const float *values, int nx, int ny, int nz, float iso,
                    const int32_t *vert_edge, int64_t n_vert, int steps, float *positions, float *normals, void *stream) {
    if (n_vert < 0) return fail(DSDF_ERR_INVALID_ARG, "dsdf_iso_refine: negative vertex count");
    if (steps < 1 || steps > 32) return fail(DSDF_ERR_INVALID_ARG, "dsdf_iso_refine: steps must be 1 ... 32");
    if (rx < 1 || ry < 1 || rz < 1) return fail(DSDF_ERR_INVALID_ARG, "dsdf_iso_refine: bad grid size");
    if (int rc = iso_check_lattice("dsdf_iso_refine", nx, ny, nz)) return rc;
    if (n_vert == 0) return DSDF_OK;
    if (!padded || !values || !vert_edge || !positions) return fail(DSDF_ERR_INVALID_ARG, "dsdf_iso_refine: null pointer argument");
    if (n_vert > 7 * iso_node_count(nx, ny, nz)) return fail(DSDF_ERR_INVALID_ARG, "dsdf_iso_refine: more vertices than the lattice has edges");
    return launch_lanes("k_iso_refine", k_iso_refine, n_vert, (hipStream_t)stream, iso_view(padded, rx, ry, rz),
                  iso_lattice(nx, ny, nz), values, iso, vert_edge, n_vert, steps, positions, normals);
}

int dsdf_volume_sample(const float *volume, int vx, int vy, int vz, int channels, const float *points, int64_t n, float *out, void *stream) {
    if (channels != 1 && channels != 3) return fail(DSDF_ERR_INVALID_ARG, "dsdf_volume_sample: channels must be 1 or 3");
    if (vx < 1 || vy < 1 || vz < 1) return fail(DSDF_ERR_INVALID_ARG, "dsdf_volume_sample: bad volume size");
    if (n < 0 || n > (int64_t)256 * 0x7fffffff) return fail(DSDF_ERR_INVALID_ARG, "dsdf_volume_sample: bad point count");
    if (!volume) return fail(DSDF_ERR_INVALID_ARG, "dsdf_volume_sample: null pointer argument");
    if (n == 0) return DSDF_OK;
    if (!points || !out) return fail(DSDF_ERR_INVALID_ARG, "dsdf_volume_sample: null pointer argument");
    AlbedoView A;
    A.data = volume; A.rx = vx; A.ry = vy; A.rz = vz;
    return launch_lanes("k_volume_sample", k_volume_sample, n, (hipStream_t)stream, A, channels, points, n, out);
}

}  // extern "C"
#endif  // __HIPCC__
