// TEST-ONLY host build of the mesh's connected components (csrc/dsdf_components.h): the statements of the kernels run serially on the CPU,
// the compare-and-swap and the atomic load of the device being plain statements here (the header's macro seam).  The CPU test-suite
// compares it with a numpy union-find, the GPU tests expect the device to return its numbers and bits; `main` runs a case file and serves
// the sanitizer build.  It is NOT a fallback: the product only ever loads the HIP library.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../differentiable-sdf-rendering_amd/csrc/dsdf_components.h"

using namespace dsdf;

extern "C" {

// What dsdf_mesh_components does, its refusals included (-1): k_cc_init, k_cc_hook, k_cc_flatten in the order of the indices.
int components_host(const int32_t *faces, long n_faces, int n_vertices, int32_t *label, int32_t *status) {
    if (n_vertices == 0) return 0;
    if (n_vertices < 0 || n_faces < 0 || n_faces > 0x7fffffffL / 3 || !label || !status || (n_faces > 0 && !faces)) return -1;
    const int64_t cap = (int64_t)n_vertices + 1;
    for (int v = 0; v < n_vertices; ++v) label[v] = v;
    if (n_faces == 0) return 0;
    for (long f = 0; f < n_faces; ++f) cc_hook_face(faces, f, label, cap, status);
    for (int v = 0; v < n_vertices; ++v) cc_flatten_vertex(label, v, cap, status);
    return 0;
}

// What dsdf_mesh_face_measures does.
int face_measures_host(const float *vert, const int32_t *faces, long n_faces, float *area, float *vol) {
    if (n_faces == 0) return 0;
    if (!vert || !faces || !area || !vol || n_faces < 0 || n_faces > 0x7fffffffL / 3) return -1;
    for (long f = 0; f < n_faces; ++f) cc_face_measures(vert, faces, f, area, vol);
    return 0;
}

// One walk with the kernels' cap on a label array of the caller's making: the root, or -1 with *status = 1 where there is none.
int root_host(int32_t *label, int v, int n_vertices, int32_t *status) { return cc_root(label, v, (int64_t)n_vertices + 1, status); }

// One union with the kernels' cap, likewise.
void union_host(int32_t *label, int a, int b, int n_vertices, int32_t *status) { cc_union(label, a, b, (int64_t)n_vertices + 1, status); }

}  // extern "C"

// `prog case.bin`: int32 V, int32 F, then 3 V floats, 3 F int32.  Labels the mesh and compares with labels found another way (the minimum
// of a face's three labels handed to all three, swept over the faces until nothing changes); checks the per-face measures for being
// finite wherever the vertices are; then the give-up path on a label array with a cycle, and the refusals.  Exit status 1 on a mismatch.
int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) { perror(argv[1]); return 2; }
    int32_t hd[2];
    if (fread(hd, 4, 2, fh) != 2 || hd[0] < 0 || hd[1] < 0) { fprintf(stderr, "bad header\n"); return 2; }
    const int V = hd[0], F = hd[1];
    std::vector<float> vert((size_t)3 * V);
    std::vector<int32_t> faces((size_t)3 * F);
    if (fread(vert.data(), 4, vert.size(), fh) != vert.size() || fread(faces.data(), 4, faces.size(), fh) != faces.size()) {
        fprintf(stderr, "truncated case file\n");
        return 2;
    }
    fclose(fh);
    std::vector<int32_t> label(V, -7), want(V);
    std::vector<float> area(F), vol(F);
    int32_t status = 0;
    long bad = 0;
    bad += components_host(faces.data(), F, V, label.data(), &status) != 0;
    bad += status != 0;
    bad += face_measures_host(vert.data(), faces.data(), F, area.data(), vol.data()) != 0;
    for (int v = 0; v < V; ++v) want[v] = v;
    for (bool changed = true; changed;) {
        changed = false;
        for (int pass = 0; pass < 2; ++pass)
            for (long g = 0; g < F; ++g) {
                const long f = pass ? F - 1 - g : g;
                int32_t *t = faces.data() + 3 * f;
                const int32_t m = std::min(want[t[0]], std::min(want[t[1]], want[t[2]]));
                for (int k = 0; k < 3; ++k)
                    if (want[t[k]] != m) { want[t[k]] = m; changed = true; }
            }
    }
    for (int v = 0; v < V; ++v) bad += label[v] != want[v];
    long components = 0;
    {
        std::vector<char> has(V, 0);
        for (long f = 0; f < F; ++f) has[label[faces[3 * f]]] = 1;
        for (int v = 0; v < V; ++v) components += has[v];
    }
    for (long f = 0; f < F; ++f) bad += !(area[f] >= 0.f && area[f] < INFINITY && vol[f] - vol[f] == 0.f);
    // the give-up path: 0 -> 1 -> 2 -> 0 is no forest
    int32_t cyc[3] = {1, 2, 0}, st = 0;
    bad += root_host(cyc, 0, 3, &st) != -1 || st != 1;
    st = 0;
    union_host(cyc, 0, 2, 3, &st);
    bad += st != 1 || cyc[0] != 1 || cyc[1] != 2 || cyc[2] != 0;
    bad += components_host(faces.data(), -1, 4, label.data(), &status) != -1;
    bad += components_host(nullptr, 1, 4, label.data(), &status) != -1;
    bad += components_host(faces.data(), 0, -1, label.data(), &status) != -1;
    bad += components_host(nullptr, 5, 0, nullptr, nullptr) != 0;
    printf("%d vertices, %d faces -> %ld components, %ld mismatches\n", V, F, components, bad);
    return bad ? 1 : 0;
}
