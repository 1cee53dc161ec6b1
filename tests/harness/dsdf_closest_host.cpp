// TEST-ONLY host build of the closest-point arithmetic of the mesh BVH (csrc/dsdf_bvh.h): tri_closest, box_dist2 and the stackless
// descent bvh_closest, run serially on the CPU next to the loop over all triangles that k_mesh_closest runs.  The CPU test-suite checks
// that the two return the same bits and compares them with an fp64 reference; `main` does the bitwise comparison for a case file and
// serves the sanitizer build.  It is NOT a fallback: the product only ever loads the HIP library.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>
#include "../../differentiable-sdf-rendering_amd/csrc/dsdf_bvh.h"

using namespace dsdf;

// what closest_store (the kernels' epilogue) writes
static void store(BvhClosest r, const float *p, float max_dist, long i, float *dist, int32_t *prim, float *point, float *bary) {
    dist[i] = closest_dist(r, max_dist);
    prim[i] = r.prim;
    const bool found = r.prim >= 0;
    const V3 q = found ? tri_point(p, r.u, r.v) : mk(0.f, 0.f, 0.f);
    point[3 * i] = q.x; point[3 * i + 1] = q.y; point[3 * i + 2] = q.z;
    bary[2 * i] = found ? r.u : 0.f; bary[2 * i + 1] = found ? r.v : 0.f;
}

extern "C" {

long closest_host_size(int n_tri) { return (long)bvh_floats(n_tri, 0); }

// the library's build (dsdf_mesh_bvh_build), serially; order = NULL: Morton order of the centroids, ties in index order
void closest_host_build(const float *tri, const int32_t *order, int n_tri, float *bvh) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long e = 0; e < (long)n_tri * 3; ++e)
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], tri[3 * e + a]); hi[a] = fmaxf(hi[a], tri[3 * e + a]); }
    std::vector<int32_t> morton;
    if (!order) {
        std::vector<int32_t> codes(n_tri);
        for (int t = 0; t < n_tri; ++t) codes[t] = bvh_morton(tri + (size_t)9 * t, lo, hi);
        morton.resize(n_tri);
        std::iota(morton.begin(), morton.end(), 0);
        std::stable_sort(morton.begin(), morton.end(), [&](int32_t a, int32_t b) { return codes[a] < codes[b]; });
        order = morton.data();
    }
    bvh_write_header(bvh, n_tri, 0, lo, hi);
    const int L = bvh_leaves(n_tri);
    for (int j = 0; j < L; ++j) bvh_write_leaf(bvh, tri, nullptr, order, j);
    for (uint32_t count = (uint32_t)L >> 1; count >= 2; count >>= 1)
        for (uint32_t k = 0; k < count; ++k) bvh_fit_node(bvh, count - 1u + k);
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
        store(r, p, max_dist, i, dist, prim, point, bary);
    }
}

// the loop of k_mesh_closest over the same triangle function, in index order
void closest_host_brute(const float *tri, int n_tri, const float *pts, long n, float max_dist, float *dist, int32_t *prim, float *point,
                        float *bary) {
    for (long i = 0; i < n; ++i) {
        const V3 x = mk(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
        BvhClosest r;
        r.d2 = closest_bound(max_dist); r.prim = -1; r.slot = 0; r.u = 0.f; r.v = 0.f;
        for (int k = 0; k < n_tri; ++k) {
            TriClosest c;
            tri_closest(tri + (size_t)9 * k, x, c);
            closest_update(r, c, k, 0);
        }
        store(r, tri + (size_t)9 * (r.prim >= 0 ? r.prim : 0), max_dist, i, dist, prim, point, bary);
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
    if (argc < 2) { fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t T = 0, n = 0;
    float max_dist = 0.f;
    if (fread(&T, 4, 1, f) != 1 || fread(&n, 4, 1, f) != 1 || fread(&max_dist, 4, 1, f) != 1 || T < 1 || n < 0) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<float> tri((size_t)9 * T), pts((size_t)3 * n);
    if (fread(tri.data(), 4, tri.size(), f) != tri.size() || fread(pts.data(), 4, pts.size(), f) != pts.size()) { fprintf(stderr, "truncated case file\n"); return 2; }
    fclose(f);
    std::vector<float> d0(n), q0((size_t)3 * n), b0((size_t)2 * n), d1(n), q1((size_t)3 * n), b1((size_t)2 * n);
    std::vector<int32_t> p0(n), p1(n), given(T);
    std::iota(given.begin(), given.end(), 0);
    closest_host_brute(tri.data(), T, pts.data(), n, max_dist, d1.data(), p1.data(), q1.data(), b1.data());
    long bad = 0, found = 0;
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<float> bvh((size_t)closest_host_size(T));
        closest_host_build(tri.data(), pass ? nullptr : given.data(), T, bvh.data());
        closest_host_bvh(bvh.data(), pts.data(), n, max_dist, d0.data(), p0.data(), q0.data(), b0.data());
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
