// TEST-ONLY host build of the mesh simplification (csrc/dsdf_simplify.h): the statements of the four kernels run serially on the CPU, with
// std::stable_sort and plain loops where the product uses torch.sort / unique_consecutive / cumsum.  The CPU test-suite compares it with
// an fp64 reference in another formulation, the GPU tests expect the device to return its bits; `main` runs a case file and serves the
// sanitizer build.  It is NOT a fallback: the product only ever loads the HIP library.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>
#include "../../differentiable-sdf-rendering_amd/csrc/dsdf_simplify.h"

using namespace dsdf;

extern "C" {

// What dsdf_simplify_keys / _mark / _emit do between them, their refusals included: -1 with the reason in `why` (unless NULL).
// keys_out 3 F; faces_out up to F x 3; pos_out / nrm_out / col_out up to 3 F x 3 (nrm_out, col_out and colors may be NULL); counts[0] = the
// number of output vertices, counts[1] = of output faces, counts[2] = of occupied cells.
int simplify_host(const float *vert, const int32_t *faces, long n_faces, const float *colors, const float *lo, const float *hi, int cx, int cy, int cz,
                  float reg, int32_t *keys_out, int32_t *faces_out, float *pos_out, float *nrm_out, float *col_out, long *counts, const char **why) {
    SimplifyGrid G;
    const char *bad = simplify_grid(lo, hi, cx, cy, cz, G);
    if (!bad && !(reg > 0.f && reg < INFINITY)) bad = "reg must be > 0";
    if (!bad && !counts) bad = "bad argument";
    if (!bad && n_faces != 0 && (!vert || !faces || !keys_out || !faces_out || !pos_out || n_faces < 0 || n_faces > 0x7fffffffL / 3 || (col_out && !colors)))
        bad = "bad argument";
    if (why) *why = bad;
    if (bad) return -1;
    counts[0] = counts[1] = counts[2] = 0;
    if (n_faces == 0) return 0;
    const long n = 3 * n_faces;
    for (long e = 0; e < n; ++e) keys_out[e] = simplify_key(G, vert + 3 * (size_t)faces[e]);                // k_simplify_keys
    std::vector<int32_t> corner(n);
    std::iota(corner.begin(), corner.end(), 0);
    std::stable_sort(corner.begin(), corner.end(), [&](int32_t a, int32_t b) { return keys_out[a] < keys_out[b]; });
    std::vector<int32_t> cell_keys, cell_start;
    for (long s = 0; s < n; ++s)
        if (s == 0 || keys_out[corner[s]] != keys_out[corner[s - 1]]) { cell_keys.push_back(keys_out[corner[s]]); cell_start.push_back((int32_t)s); }
    cell_start.push_back((int32_t)n);
    const int U = (int)cell_keys.size();
    std::vector<int32_t> rank(n), keep(n_faces), used(U, 0), vid(U), foff(n_faces);
    for (long f = 0; f < n_faces; ++f) simplify_mark_face(keys_out, f, cell_keys.data(), U, rank.data(), keep.data(), used.data());   // k_simplify_mark
    int32_t nv = 0, nf = 0;
    for (int r = 0; r < U; ++r) { vid[r] = nv; nv += used[r]; }
    for (long f = 0; f < n_faces; ++f) { foff[f] = nf; nf += keep[f]; }
    for (long f = 0; f < n_faces; ++f)                                                                       // k_simplify_faces
        if (keep[f]) for (int k = 0; k < 3; ++k) faces_out[3 * (size_t)foff[f] + k] = vid[rank[3 * f + k]];
    for (int r = 0; r < U; ++r) {                                                                            // k_simplify_cells
        if (!used[r]) continue;
        const size_t o = 3 * (size_t)vid[r];
        simplify_cell(G, reg, vert, faces, colors, corner.data(), cell_start[r], cell_start[r + 1], cell_keys[r], pos_out + o, nrm_out ? nrm_out + o : nullptr,
                      col_out ? col_out + o : nullptr);
    }
    counts[0] = nv; counts[1] = nf; counts[2] = U;
    return 0;
}

}  // extern "C"

// `prog case.bin`: int32 V, int32 F, int32 cx, cy, cz, float lo[3], hi[3], then 3 V floats, 3 V colour floats, 3 F int32.  Simplifies with
// normals and colours and checks what must hold whatever the mesh: face indices in range and pairwise different, every vertex finite
// and inside the box (a NaN vertex lands in a cell like any other), unit or zero normals; then the refusals.  Exit status 1 on a failure.
int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) { perror(argv[1]); return 2; }
    int32_t hd[5];
    float box[6];
    if (fread(hd, 4, 5, fh) != 5 || fread(box, 4, 6, fh) != 6 || hd[0] < 1 || hd[1] < 0) { fprintf(stderr, "bad header\n"); return 2; }
    const int V = hd[0], F = hd[1];
    std::vector<float> vert((size_t)3 * V), colors((size_t)3 * V);
    std::vector<int32_t> faces((size_t)3 * F);
    if (fread(vert.data(), 4, vert.size(), fh) != vert.size() || fread(colors.data(), 4, colors.size(), fh) != colors.size() ||
        fread(faces.data(), 4, faces.size(), fh) != faces.size()) { fprintf(stderr, "truncated case file\n"); return 2; }
    fclose(fh);
    std::vector<int32_t> keys((size_t)3 * F), fo((size_t)3 * F);
    std::vector<float> pos((size_t)9 * F), nrm((size_t)9 * F), col((size_t)9 * F);
    long counts[3];
    const char *why = nullptr;
    if (simplify_host(vert.data(), faces.data(), F, colors.data(), box, box + 3, hd[2], hd[3], hd[4], DSDF_SIMPLIFY_REG, keys.data(), fo.data(), pos.data(),
                      nrm.data(), col.data(), counts, &why)) { fprintf(stderr, "refused: %s\n", why); return 1; }
    long bad = 0;
    for (long f = 0; f < counts[1]; ++f) {
        const int32_t *t = fo.data() + 3 * f;
        bad += !(t[0] >= 0 && t[1] >= 0 && t[2] >= 0 && t[0] < counts[0] && t[1] < counts[0] && t[2] < counts[0] && t[0] != t[1] && t[1] != t[2] && t[2] != t[0]);
    }
    for (long v = 0; v < counts[0]; ++v) {
        for (int a = 0; a < 3; ++a) {
            const float x = pos[3 * v + a], m = 1e-5f * (box[3 + a] - box[a]);
            bad += !(x >= box[a] - m && x <= box[3 + a] + m);
        }
        const float *q = nrm.data() + 3 * v;
        const float l = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
        bad += !(l == 0.f || fabsf(l - 1.f) < 1e-5f);
    }
    float nolo[3] = {0.f, 0.f, 0.f}, nohi[3] = {1.f, 0.f, 1.f};
    bad += simplify_host(vert.data(), faces.data(), F, nullptr, nolo, nohi, 2, 2, 2, 1e-3f, keys.data(), fo.data(), pos.data(), nullptr, nullptr, counts, nullptr) != -1;
    bad += simplify_host(vert.data(), faces.data(), F, nullptr, box, box + 3, 2048, 1024, 1024, 1e-3f, keys.data(), fo.data(), pos.data(), nullptr, nullptr, counts, nullptr) != -1;
    printf("%d vertices, %d faces -> %ld vertices, %ld faces, %ld failures\n", V, F, counts[0], counts[1], bad);
    return bad ? 1 : 0;
}
