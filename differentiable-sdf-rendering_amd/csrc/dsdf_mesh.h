// dsdf_mesh.h -- the brute-force mesh queries (included by dsdf_kernels.hip after dsdf_bvh.h): closest-hit ray casting, the one native
// operation `mesh_to_sdf.create_sdf` (python/mesh_to_sdf.py:9-57) takes from Mitsuba (`scene.ray_intersect` on an obj / ply shape), and
// closest-point queries; dsdf_winding.h adds the winding number on the same loop.
// Asset preparation, not the per-iteration hot path: brute force, N-body style -- a block stages DSDF_MESH_TILE triangles in
// LDS (36 B each, read as broadcasts) and every thread visits them in index order (mesh_for_each_triangle, the one statement of that
// loop).  What a thread does with one triangle is a host/device function of dsdf_bvh.h / dsdf_winding.h (ray_best_update, tri_closest +
// closest_update, tri_solid_angle), shared with the BVH traversals that serve large meshes and with the host tests; rays x triangles
// tests at ~10^12 / s: 128^3 voxel-centre rays x 20 k triangles in a fraction of a second, the 256-direction refinement of a 256^3 grid
// against 100 k triangles in tens of seconds.
#pragma once

#define DSDF_MESH_TILE 256

// tri: n_tri x 9 floats (p0, p1, p2); tile: the block's own __shared__ float[DSDF_MESH_TILE * 9].  Calls body(p, index) for every
// triangle, in index order, p pointing at its nine floats in LDS.  ALL threads of the block call this, those without an element of
// their own included: the two barriers per tile are the block's.  tid, nthr: the caller's threadIdx.x and blockDim.x (the defaults
// are evaluated in the kernel); as plain unsigned arguments the staging loop compiles to what it did when each kernel spelled it out.
template <class Body>
__device__ __forceinline__ void mesh_for_each_triangle(const float *__restrict__ tri, int n_tri, float *tile, Body body,
                                                       unsigned tid = threadIdx.x, unsigned nthr = blockDim.x) {
    for (int t0 = 0; t0 < n_tri; t0 += DSDF_MESH_TILE) {
        const int cnt = min(DSDF_MESH_TILE, n_tri - t0);
        __syncthreads();
        for (int e = tid; e < cnt * 9; e += nthr) tile[e] = tri[(size_t)t0 * 9 + e];
        __syncthreads();
        for (int k = 0; k < cnt; ++k) body(tile + k * 9, t0 + k);
    }
}

// t_out: distance of the closest hit with t > t_min (inf: none); back_out: 1 when the geometric normal (p1 - p0) x (p2 - p0) of that
// triangle points along the ray, i.e. the ray leaves the solid through it.  (The index of the triangle is not reported.)
__global__ __launch_bounds__(256) void k_mesh_raycast(const float *__restrict__ tri, int n_tri, const float *__restrict__ ro,
                                                      const float *__restrict__ rd, int64_t n, float t_min,
                                                      float *__restrict__ t_out, int32_t *__restrict__ back_out) {
    __shared__ float tile[DSDF_MESH_TILE * 9];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = i < n;
    V3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 1.f, 0.f);
    if (on) { o = mk(ro[3 * i], ro[3 * i + 1], ro[3 * i + 2]); d = mk(rd[3 * i], rd[3 * i + 1], rd[3 * i + 2]); }
    RayBest b;
    ray_best_init(b);
    mesh_for_each_triangle(tri, n_tri, tile, [&b, o, d, t_min](const float *p, int k) { ray_best_update(b, p, o, d, t_min, k); });
    if (on) { t_out[i] = b.t; if (back_out) back_out[i] = b.back; }
}

extern "C" int dsdf_mesh_raycast(const float *triangles, int n_triangles, const float *rays_o, const float *rays_d, int64_t n,
                                 float t_min, float *t_out, int32_t *backface_out, void *stream) {
    if (n == 0) return DSDF_OK;
    if (!triangles || n_triangles < 1 || !rays_o || !rays_d || !t_out || n < 0) return fail(DSDF_ERR_INVALID_ARG, "dsdf_mesh_raycast: bad argument");
    return launch_lanes("k_mesh_raycast", k_mesh_raycast, n, (hipStream_t)stream, triangles, n_triangles, rays_o, rays_d, n, t_min, t_out,
                        backface_out);
}

// ---- closest point -------------------------------------------------------------------------------------------------------
// The same loop for closest-point queries (tri_closest, dsdf_bvh.h): in index order, so `closest_update` keeps the lowest index among
// equal distances.  It serves small meshes, and on the device it is the yardstick of the traversal (k_mesh_bvh_closest returns the
// same bits).
__global__ __launch_bounds__(256) void k_mesh_closest(const float *__restrict__ tri, int n_tri, const float *__restrict__ pts, int64_t n,
                                                      float max_dist, float *__restrict__ dist_out, int32_t *__restrict__ prim_out,
                                                      float *__restrict__ point_out, float *__restrict__ bary_out) {
    __shared__ float tile[DSDF_MESH_TILE * 9];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = i < n;
    V3 x = mk(0.f, 0.f, 0.f);
    if (on) x = mk(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    BvhClosest r;
    closest_init(r, closest_bound(max_dist));
    mesh_for_each_triangle(tri, n_tri, tile, [&r, x](const float *p, int k) {
        TriClosest c;
        tri_closest(p, x, c);
        closest_update(r, c, k, 0);
    });
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
    return launch_lanes("k_mesh_closest", k_mesh_closest, n, (hipStream_t)stream, triangles, n_triangles, points, n, max_dist, dist_out,
                        prim_out, point_out, bary_out);
}
