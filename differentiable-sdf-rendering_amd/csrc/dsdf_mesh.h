// dsdf_mesh.h -- closest-hit ray / triangle-soup casting (included by dsdf_kernels.hip): the one native operation
// `mesh_to_sdf.create_sdf` (python/mesh_to_sdf.py:9-57) takes from Mitsuba (`scene.ray_intersect` on an obj / ply shape).
// Asset preparation, not the per-iteration hot path: brute force, N-body style -- a block stages DSDF_MESH_TILE triangles in
// LDS (36 B each, read as broadcasts) and every thread tests its ray against them (tri_intersect, dsdf_bvh.h: the one statement of
// the triangle test, shared with the BVH traversal that serves large meshes); rays x triangles tests at ~10^12 / s: 128^3 voxel-centre rays x 20 k triangles in a fraction of a second, the
// 256-direction refinement of a 256^3 grid against 100 k triangles in tens of seconds.
#pragma once

#define DSDF_MESH_TILE 256

// tri: n_tri x 9 floats (p0, p1, p2).  t_out: distance of the closest hit with t > t_min (inf: none); back_out: 1 when the
// geometric normal (p1 - p0) x (p2 - p0) of that triangle points along the ray, i.e. the ray leaves the solid through it.
__global__ __launch_bounds__(256) void k_mesh_raycast(const float *__restrict__ tri, int n_tri, const float *__restrict__ ro,
                                                      const float *__restrict__ rd, int64_t n, float t_min,
                                                      float *__restrict__ t_out, int32_t *__restrict__ back_out) {
    __shared__ float tile[DSDF_MESH_TILE * 9];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = i < n;
    V3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 1.f, 0.f);
    if (on) { o = mk(ro[3 * i], ro[3 * i + 1], ro[3 * i + 2]); d = mk(rd[3 * i], rd[3 * i + 1], rd[3 * i + 2]); }
    float best = INFINITY;
    int back = 0;
    for (int t0 = 0; t0 < n_tri; t0 += DSDF_MESH_TILE) {
        const int cnt = min(DSDF_MESH_TILE, n_tri - t0);
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * 9; e += blockDim.x) tile[e] = tri[(size_t)t0 * 9 + e];
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {
            TriHit h;
            if (tri_intersect(tile + k * 9, o, d, h) && h.t > t_min && h.t < best) {
                best = h.t;
                back = h.det < 0.f ? 1 : 0;        // det = e1 . (d x e2) = -d . (e1 x e2): negative when the normal points along the ray
            }
        }
    }
    if (on) { t_out[i] = best; if (back_out) back_out[i] = back; }
}

extern "C" int dsdf_mesh_raycast(const float *triangles, int n_triangles, const float *rays_o, const float *rays_d, int64_t n,
                                 float t_min, float *t_out, int32_t *backface_out, void *stream) {
    if (n == 0) return DSDF_OK;
    if (!triangles || n_triangles < 1 || !rays_o || !rays_d || !t_out || n < 0) return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_raycast: bad argument");
    hipLaunchKernelGGL(k_mesh_raycast, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, triangles, n_triangles, rays_o,
                       rays_d, n, t_min, t_out, backface_out);
    return check_launch("k_mesh_raycast");
}

// ---- closest point -------------------------------------------------------------------------------------------------------
// The same shape for closest-point queries (tri_closest, dsdf_bvh.h): every thread tests its point against the staged triangles,
// in index order, so `closest_update` keeps the lowest index among equal distances.  It serves small meshes, and on the device it
// is the yardstick of the traversal (k_mesh_bvh_closest returns the same bits).
__global__ __launch_bounds__(256) void k_mesh_closest(const float *__restrict__ tri, int n_tri, const float *__restrict__ pts, int64_t n,
                                                      float max_dist, float *__restrict__ dist_out, int32_t *__restrict__ prim_out,
                                                      float *__restrict__ point_out, float *__restrict__ bary_out) {
    __shared__ float tile[DSDF_MESH_TILE * 9];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = i < n;
    V3 x = mk(0.f, 0.f, 0.f);
    if (on) x = mk(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    BvhClosest r;
    r.d2 = closest_bound(max_dist); r.prim = -1; r.slot = 0; r.u = 0.f; r.v = 0.f;
    for (int t0 = 0; t0 < n_tri; t0 += DSDF_MESH_TILE) {
        const int cnt = min(DSDF_MESH_TILE, n_tri - t0);
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * 9; e += blockDim.x) tile[e] = tri[(size_t)t0 * 9 + e];
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {
            TriClosest c;
            tri_closest(tile + k * 9, x, c);
            closest_update(r, c, t0 + k, 0);
        }
    }
    if (!on) return;
    float p[9];
    const float *src = tri + (size_t)9 * (r.prim >= 0 ? r.prim : 0);
    for (int e = 0; e < 9; ++e) p[e] = src[e];
    closest_store(r, p, max_dist, i, dist_out, prim_out, point_out, bary_out);
}

extern "C" int dsdf_mesh_closest(const float *triangles, int n_triangles, const float *points, int64_t n, float max_dist, float *dist_out,
                                 int32_t *prim_out, float *point_out, float *bary_out, void *stream) {
    if (n == 0) return DSDF_OK;
    if (!triangles || n_triangles < 1 || !points || !dist_out || n < 0 || !(max_dist >= 0.f))
        return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_closest: bad argument");
    return launch("k_mesh_closest", k_mesh_closest, dim3((unsigned)((n + 255) / 256)), dim3(256), (hipStream_t)stream, triangles, n_triangles,
                  points, n, max_dist, dist_out, prim_out, point_out, bary_out);
}
