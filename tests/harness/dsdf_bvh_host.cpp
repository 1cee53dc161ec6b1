// TEST-ONLY host build of the mesh BVH arithmetic (csrc/dsdf_bvh.h): the builder's per-element statements, the stackless
// traversal and the shared triangle test, run serially on the CPU.  The CPU test-suite checks that the traversal returns bit for
// bit what a loop over all triangles returns; `main` does the same for a case file and serves the sanitizer build.  It is NOT a
// fallback: the product only ever loads the HIP library.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>
#include "../../differentiable-sdf-rendering_amd/csrc/dsdf_bvh.h"

using namespace dsdf;

extern "C" {

long bvh_host_size(int n_tri, int has_normals) { return (long)bvh_floats(n_tri, has_normals); }

void bvh_host_morton(const float *tri, int n_tri, int32_t *codes) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long e = 0; e < (long)n_tri * 3; ++e)
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], tri[3 * e + a]); hi[a] = fmaxf(hi[a], tri[3 * e + a]); }
    for (int t = 0; t < n_tri; ++t) codes[t] = bvh_morton(tri + (size_t)9 * t, lo, hi);
}

// the library's build (dsdf_mesh_bvh_build), serially
void bvh_host_build(const float *tri, const float *nrm, const int32_t *order, int n_tri, float *bvh) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long e = 0; e < (long)n_tri * 3; ++e)
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], tri[3 * e + a]); hi[a] = fmaxf(hi[a], tri[3 * e + a]); }
    bvh_write_header(bvh, n_tri, nrm != nullptr, lo, hi);
    const int L = bvh_leaves(n_tri);
    for (int j = 0; j < L; ++j) bvh_write_leaf(bvh, tri, nrm, order, j);
    for (uint32_t count = (uint32_t)L >> 1; count >= 2; count >>= 1)
        for (uint32_t k = 0; k < count; ++k) bvh_fit_node(bvh, count - 1u + k);
}

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

// the loop of k_mesh_raycast over the same triangle function (strict `<` in index order: the lowest index wins a tie)
void bvh_host_brute(const float *tri, int n_tri, const float *ro, const float *rd, long n, float t_min, float *t, int32_t *back, int32_t *prim) {
    for (long i = 0; i < n; ++i) {
        const V3 o = mk(ro[3 * i], ro[3 * i + 1], ro[3 * i + 2]), d = mk(rd[3 * i], rd[3 * i + 1], rd[3 * i + 2]);
        float best = INFINITY;
        int b = 0, pr = -1;
        for (int k = 0; k < n_tri; ++k) {
            TriHit h;
            if (tri_intersect(tri + (size_t)9 * k, o, d, h) && h.t > t_min && h.t < best) { best = h.t; b = h.det < 0.f ? 1 : 0; pr = k; }
        }
        t[i] = best; back[i] = b; prim[i] = pr;
    }
}

}  // extern "C"

// `prog case.bin`: int32 T, int32 n, float t_min, 9 T floats, 3 n origins, 3 n directions.  Builds the BVH in Morton order,
// casts the rays both ways and compares bit for bit; exit status 1 on a mismatch.
int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t T = 0, n = 0;
    float t_min = 0.f;
    if (fread(&T, 4, 1, f) != 1 || fread(&n, 4, 1, f) != 1 || fread(&t_min, 4, 1, f) != 1 || T < 1 || n < 0) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<float> tri((size_t)9 * T), ro((size_t)3 * n), rd((size_t)3 * n);
    if (fread(tri.data(), 4, tri.size(), f) != tri.size() || fread(ro.data(), 4, ro.size(), f) != ro.size() ||
        fread(rd.data(), 4, rd.size(), f) != rd.size()) { fprintf(stderr, "truncated case file\n"); return 2; }
    fclose(f);
    std::vector<int32_t> codes(T), order(T);
    bvh_host_morton(tri.data(), T, codes.data());
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return codes[a] < codes[b]; });
    std::vector<float> bvh((size_t)bvh_host_size(T, 0));
    bvh_host_build(tri.data(), nullptr, order.data(), T, bvh.data());
    std::vector<float> t0(n), t1(n);
    std::vector<int32_t> b0(n), b1(n), p0(n), p1(n);
    bvh_host_raycast(bvh.data(), ro.data(), rd.data(), n, t_min, t0.data(), b0.data(), p0.data());
    bvh_host_brute(tri.data(), T, ro.data(), rd.data(), n, t_min, t1.data(), b1.data(), p1.data());
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
