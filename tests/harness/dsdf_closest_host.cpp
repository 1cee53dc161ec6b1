// TEST-ONLY host build of the closest-point arithmetic of the mesh BVH (csrc/dsdf_bvh.h): tri_closest, box_dist2 and the stackless
// descent bvh_closest, run serially on the CPU next to the loop over all triangles made of the statements k_mesh_closest runs
// (closest_init, tri_closest + closest_update per triangle, closest_store -- the kernels' own epilogue).  The CPU test-suite checks
// that the two return the same bits and compares them with an fp64 reference; `main` does the bitwise comparison for a case file and
// serves the sanitizer build.  It is NOT a fallback: the product only ever loads the HIP library.
#include "dsdf_mesh_host.h"

using namespace dsdf;

extern "C" {

long closest_host_size(int n_tri) { return (long)bvh_floats(n_tri, 0); }

// the library's build (dsdf_mesh_bvh_build), serially; order = NULL: Morton order of the centroids, ties in index order
void closest_host_build(const float *tri, const int32_t *order, int n_tri, float *bvh) {
    std::vector<int32_t> morton;
    if (!order) { morton = host_morton_order(tri, n_tri); order = morton.data(); }
    host_bvh_build(tri, nullptr, order, n_tri, bvh);
}

void closest_host_bvh(const float *bvh, const float *pts, long n, float max_dist, float *dist, int32_t *prim, float *point, float *bary) {
    const BvhView B = bvh_view(bvh);
    GlobalNodes N;
    N.nodes = B.nodes;
    for (long i = 0; i < n; ++i) {
        BvhClosest r;
        bvh_closest(B, N, mk(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]), closest_bound(max_dist), r);
        float p[DSDF_BVH_SLOT];
        bvh_load_slot(B, r.slot, p);
        closest_store(r, p, max_dist, i, dist, prim, point, bary);
    }
}

// the loop of k_mesh_closest, in index order
void closest_host_brute(const float *tri, int n_tri, const float *pts, long n, float max_dist, float *dist, int32_t *prim, float *point,
                        float *bary) {
    for (long i = 0; i < n; ++i) {
        const V3 x = mk(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
        BvhClosest r;
        closest_init(r, closest_bound(max_dist));
        for (int k = 0; k < n_tri; ++k) {
            TriClosest c;
            tri_closest(tri + (size_t)9 * k, x, c);
            closest_update(r, c, k, 0);
        }
        closest_store(r, tri + (size_t)9 * (r.prim >= 0 ? r.prim : 0), max_dist, i, dist, prim, point, bary);
    }
}

// one triangle each: (d2, u, v) of tri_closest for point i against triangle i
void closest_host_tri(const float *tri, const float *pts, long n, float *d2uv) {
    for (long i = 0; i < n; ++i) {
        TriClosest c;
        tri_closest(tri + (size_t)9 * i, mk(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]), c);
        d2uv[3 * i] = c.d2; d2uv[3 * i + 1] = c.u; d2uv[3 * i + 2] = c.v;
    }
}

}  // extern "C"

// `prog case.bin`: int32 T, int32 n, float max_dist, 9 T floats, 3 n points.  Builds the BVH in the given order and in Morton order,
// queries both and the loop over all triangles, and compares bit for bit; exit status 1 on a mismatch.
int main(int argc, char **argv) {
    HostCase c;
    if (int rc = host_read_case(argc, argv, 1, c)) return rc;
    const int T = c.T, n = c.n;
    const float max_dist = c.scalar, *tri = c.tri.data(), *pts = c.blocks[0].data();
    std::vector<float> d0(n), q0((size_t)3 * n), b0((size_t)2 * n), d1(n), q1((size_t)3 * n), b1((size_t)2 * n);
    std::vector<int32_t> p0(n), p1(n), given(T);
    std::iota(given.begin(), given.end(), 0);
    closest_host_brute(tri, T, pts, n, max_dist, d1.data(), p1.data(), q1.data(), b1.data());
    long bad = 0, found = 0;
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<float> bvh((size_t)closest_host_size(T));
        closest_host_build(tri, pass ? nullptr : given.data(), T, bvh.data());
        closest_host_bvh(bvh.data(), pts, n, max_dist, d0.data(), p0.data(), q0.data(), b0.data());
        for (int i = 0; i < n; ++i) {
            bool same = f2i(d0[i]) == f2i(d1[i]) && p0[i] == p1[i] && f2i(b0[2 * i]) == f2i(b1[2 * i]) && f2i(b0[2 * i + 1]) == f2i(b1[2 * i + 1]);
            for (int a = 0; a < 3; ++a) same = same && f2i(q0[3 * i + a]) == f2i(q1[3 * i + a]);
            if (!same && bad++ < 5) fprintf(stderr, "point %d (pass %d): bvh d %.9g prim %d, brute d %.9g prim %d\n", i, pass, d0[i], p0[i], d1[i], p1[i]);
        }
    }
    for (int i = 0; i < n; ++i) found += p1[i] >= 0;
    printf("%d triangles, %d points, %ld found, %ld mismatches\n", T, n, found, bad);
    return bad ? 1 : 0;
}
