// TEST-ONLY host build of the mesh BVH arithmetic (csrc/dsdf_bvh.h): the builder's per-element statements (dsdf_mesh_host.h runs them
// serially), the stackless traversal, and the loop over all triangles made of the statements k_mesh_raycast runs per triangle
// (ray_best_init / ray_best_update).  The CPU test-suite checks that the traversal returns bit for bit what that loop returns; `main`
// does the same for a case file and serves the sanitizer build.  It is NOT a fallback: the product only ever loads the HIP library.
#include "dsdf_mesh_host.h"

using namespace dsdf;

extern "C" {

long bvh_host_size(int n_tri, int has_normals) { return (long)bvh_floats(n_tri, has_normals); }

void bvh_host_morton(const float *tri, int n_tri, int32_t *codes) { host_morton(tri, n_tri, codes); }

// the library's build (dsdf_mesh_bvh_build), serially; order = NULL: the given order
void bvh_host_build(const float *tri, const float *nrm, const int32_t *order, int n_tri, float *bvh) { host_bvh_build(tri, nrm, order, n_tri, bvh); }

void bvh_host_raycast(const float *bvh, const float *ro, const float *rd, long n, float t_min, float *t, int32_t *back, int32_t *prim) {
    const BvhView B = bvh_view(bvh);
    GlobalNodes N;
    N.nodes = B.nodes;
    for (long i = 0; i < n; ++i) {
        BvhHit h;
        bvh_traverse<false>(B, N, mk(ro[3 * i], ro[3 * i + 1], ro[3 * i + 2]), mk(rd[3 * i], rd[3 * i + 1], rd[3 * i + 2]), t_min, INFINITY, h);
        t[i] = h.t; back[i] = (h.prim >= 0 && h.det < 0.f) ? 1 : 0; prim[i] = h.prim;
    }
}

// any-hit query with t_min < t < t_max per ray
void bvh_host_anyhit(const float *bvh, const float *ro, const float *rd, long n, float t_min, const float *t_max, int32_t *occluded) {
    const BvhView B = bvh_view(bvh);
    GlobalNodes N;
    N.nodes = B.nodes;
    for (long i = 0; i < n; ++i) {
        BvhHit h;
        occluded[i] = bvh_traverse<true>(B, N, mk(ro[3 * i], ro[3 * i + 1], ro[3 * i + 2]), mk(rd[3 * i], rd[3 * i + 1], rd[3 * i + 2]), t_min, t_max[i], h) ? 1 : 0;
    }
}

// the loop of k_mesh_raycast, in index order (the kernel does not store the index)
void bvh_host_brute(const float *tri, int n_tri, const float *ro, const float *rd, long n, float t_min, float *t, int32_t *back, int32_t *prim) {
    for (long i = 0; i < n; ++i) {
        const V3 o = mk(ro[3 * i], ro[3 * i + 1], ro[3 * i + 2]), d = mk(rd[3 * i], rd[3 * i + 1], rd[3 * i + 2]);
        RayBest b;
        ray_best_init(b);
        for (int k = 0; k < n_tri; ++k) ray_best_update(b, tri + (size_t)9 * k, o, d, t_min, k);
        t[i] = b.t; back[i] = b.back; prim[i] = b.prim;
    }
}

}  // extern "C"

// `prog case.bin`: int32 T, int32 n, float t_min, 9 T floats, 3 n origins, 3 n directions.  Builds the BVH in Morton order,
// casts the rays both ways and compares bit for bit; exit status 1 on a mismatch.
int main(int argc, char **argv) {
    HostCase c;
    if (int rc = host_read_case(argc, argv, 2, c)) return rc;
    const int T = c.T, n = c.n;
    const float *ro = c.blocks[0].data(), *rd = c.blocks[1].data();
    const std::vector<int32_t> order = host_morton_order(c.tri.data(), T);
    std::vector<float> bvh((size_t)bvh_host_size(T, 0));
    bvh_host_build(c.tri.data(), nullptr, order.data(), T, bvh.data());
    std::vector<float> t0(n), t1(n);
    std::vector<int32_t> b0(n), b1(n), p0(n), p1(n);
    bvh_host_raycast(bvh.data(), ro, rd, n, c.scalar, t0.data(), b0.data(), p0.data());
    bvh_host_brute(c.tri.data(), T, ro, rd, n, c.scalar, t1.data(), b1.data(), p1.data());
    long bad = 0, hits = 0;
    for (int i = 0; i < n; ++i) {
        hits += p1[i] >= 0;
        if (f2i(t0[i]) != f2i(t1[i]) || b0[i] != b1[i] || p0[i] != p1[i]) {
            if (bad++ < 5) fprintf(stderr, "ray %d: bvh t %.9g prim %d, brute t %.9g prim %d\n", i, t0[i], p0[i], t1[i], p1[i]);
        }
    }
    printf("%d triangles, %d rays, %ld hits, %ld mismatches\n", T, n, hits, bad);
    return bad ? 1 : 0;
}
