// TEST-ONLY host build of the winding-number arithmetic (csrc/dsdf_winding.h): tri_solid_angle, the per-node moments and the stackless
// walk bvh_winding, run serially on the CPU next to the loop over all triangles that k_mesh_winding runs (the sum of tri_solid_angle in
// index order); the tree is built by dsdf_mesh_host.h.  The CPU test-suite compares them with an fp64 reference in another formulation;
// `main` runs a case file and serves the sanitizer build.  It is NOT a fallback: the product only ever loads the HIP library.
#include <cmath>
#include "../../differentiable-sdf-rendering_amd/csrc/dsdf_winding.h"
#include "dsdf_mesh_host.h"

using namespace dsdf;

extern "C" {

long winding_host_size(int n_tri) { return (long)bvh_floats(n_tri, 0); }
long winding_host_moments_size(int n_tri) { return (long)winding_moment_floats(n_tri); }

// the library's two builds (dsdf_mesh_bvh_build, dsdf_mesh_bvh_moments), serially; order = NULL: Morton order of the centroids, ties in
// index order
void winding_host_build(const float *tri, const int32_t *order, int n_tri, float *bvh, float *mom) {
    std::vector<int32_t> morton;
    if (!order) { morton = host_morton_order(tri, n_tri); order = morton.data(); }
    host_bvh_build(tri, nullptr, order, n_tri, bvh);
    const int L = bvh_leaves(n_tri);
    for (int j = 0; j < L; ++j) winding_leaf_moments(bvh, mom, j);
    for (uint32_t count = (uint32_t)L >> 1; count >= 1; count >>= 1)
        for (uint32_t k = 0; k < count; ++k) winding_node_moments(mom, count - 1u + k);
}

// the loop of k_mesh_winding, in index order
void winding_host_brute(const float *tri, int n_tri, const float *pts, long n, float *w) {
    for (long i = 0; i < n; ++i) {
        const V3 x = mk(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
        float s = 0.f;
        for (int k = 0; k < n_tri; ++k) s += tri_solid_angle(tri + (size_t)9 * k, x);
        w[i] = s * DSDF_WIND_INV_4PI;
    }
}

// what dsdf_mesh_bvh_winding does, its refusal of beta < 1 included (-1)
int winding_host_bvh(const float *bvh, const float *mom, const float *pts, long n, float beta, float *w) {
    if (!(beta >= 1.f)) return -1;
    const BvhView B = bvh_view(bvh);
    for (long i = 0; i < n; ++i) w[i] = bvh_winding(B, mom, mk(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]), beta);
    return 0;
}

// one triangle each: the solid angle of triangle i at point i
void winding_host_tri(const float *tri, const float *pts, long n, float *omega) {
    for (long i = 0; i < n; ++i) omega[i] = tri_solid_angle(tri + (size_t)9 * i, mk(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
}

}  // extern "C"

// `prog case.bin`: int32 T, int32 n, float beta, 9 T floats, 3 n points.  Builds the tree and its moments in the given order and in
// Morton order, walks both at beta = inf and at beta, and compares with the loop over all triangles: the exact walk adds the same terms in
// another order (1e-4 covers that), every result of a finite point is finite; exit status 1 on a mismatch.
int main(int argc, char **argv) {
    HostCase c;
    if (int rc = host_read_case(argc, argv, 1, c)) return rc;
    const int T = c.T, n = c.n;
    const float beta = c.scalar;
    const std::vector<float> &tri = c.tri, &pts = c.blocks[0];
    std::vector<float> w0(n), w1(n), w2(n);
    std::vector<int32_t> given(T);
    std::iota(given.begin(), given.end(), 0);
    winding_host_brute(tri.data(), T, pts.data(), n, w0.data());
    if (winding_host_bvh(nullptr, nullptr, nullptr, 0, 0.5f, nullptr) != -1) { fprintf(stderr, "beta < 1 was accepted\n"); return 1; }
    long bad = 0, inside = 0;
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<float> bvh((size_t)winding_host_size(T)), mom((size_t)winding_host_moments_size(T));
        winding_host_build(tri.data(), pass ? nullptr : given.data(), T, bvh.data(), mom.data());
        winding_host_bvh(bvh.data(), mom.data(), pts.data(), n, INFINITY, w1.data());
        winding_host_bvh(bvh.data(), mom.data(), pts.data(), n, beta, w2.data());
        for (int i = 0; i < n; ++i) {
            const bool finite = std::isfinite(pts[3 * i]) && std::isfinite(pts[3 * i + 1]) && std::isfinite(pts[3 * i + 2]);
            if (!finite) continue;
            const bool same = std::isfinite(w0[i]) && std::isfinite(w2[i]) && fabsf(w1[i] - w0[i]) <= 1e-4f;
            if (!same && bad++ < 5) fprintf(stderr, "point %d (pass %d): exact walk %.9g, beta %g walk %.9g, loop %.9g\n", i, pass, w1[i], beta, w2[i], w0[i]);
        }
    }
    for (int i = 0; i < n; ++i) inside += w0[i] > 0.5f;
    printf("%d triangles, %d points, %ld inside, %ld mismatches\n", T, n, inside, bad);
    return bad ? 1 : 0;
}
