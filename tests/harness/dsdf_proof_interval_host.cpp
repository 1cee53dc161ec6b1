// dsdf_proof_interval_host.cpp -- TEST-ONLY stand-alone host build of the fine proof stages in BOTH forms (csrc/dsdf_proof.h): the
// reference loop over the whole centre ray (pixel_fine_proofs) beside the form the device runs, restricted to the stretch near the
// shape (pixel_fine_proofs_near, proof_interval), with what each of them fetches counted per pixel.  Everything else -- padding, the
// serial builds of the bounds, the entries of the fine stages -- is that of dsdf_proof_stages_host.cpp, included here.  Compiled by
// tests/proof_interval_cases.py.
#include "dsdf_proof_stages_host.cpp"

namespace {
struct Counts {
    int n[DSDF_PC_N] = {};
    void add(int what, int by = 1) { n[what] += by; }
};
struct Scene {          // the bounds of one grid, as the device holds them behind the padded grid
    std::vector<float> p, fmin, fmax, craw, cdil;
    float D[3];
    GridView G;
    BoundGrid Bmin, Bmax, Bc;
    Scene(const float *data, int rx, int ry, int rz, const dsdf_params &prm)
        : p(pad(data, rx, ry, rz)), fmin(window<false>(data, rx, ry, rz)), fmax(window<true>(data, rx, ry, rz)) {
        const BlockDims cd = block_dims(rx, ry, rz, DSDF_COARSE_SHIFT(0));
        craw.resize(cd.cells); cdil.resize(cd.cells);
        block_bounds<false>(data, rx, ry, rz, DSDF_COARSE_SHIFT(0), 1, craw.data(), cdil.data());
        psh_tap_diff_max(data, rx, ry, rz, D);
        G = make_view(p.data(), rx, ry, rz, prm);
        Bmin = bound_grid(fmin.data(), block_dims(rx, ry, rz, 0), 0, 0.5f);
        Bmax = bound_grid(fmax.data(), block_dims(rx, ry, rz, 0), 0, 0.5f);
        Bc = bound_grid(cdil.data(), cd, DSDF_COARSE_SHIFT(0), 0.f);
    }
};
}  // namespace

extern "C" {

// For the film-block pixels of one view with list[i] != 0 (bit 0: run the proofs, bit 1: with the hit proof): the two bytes of the
// reference form (ref) and of the restricted form (near), the interval (ival: ta, tb, t0, t1 -- ta > tb: empty) and, per form,
// DSDF_PC_N counters (cnt: [pixel][form][counter]).  Returns the step of the fine stages (0: off for this film); info = step of the
// walks, r of the gradient bound.
float psi_proofs(const float *data, int rx, int ry, int rz, const dsdf_params *prm, const dsdf_camera *cam, int W, int H,
                 const unsigned char *list, int third, unsigned short *ref, unsigned short *near, float *ival, int *cnt, float *info) {
    const ProofMargins M = proof_margins(cam, 1, W, rx, ry, rz);
    if (!(M.fstep > 0.f)) return 0.f;
    const Scene S(data, rx, ry, rz, *prm);
    const ValueBound vb = {third ? S.D : nullptr, M.reach};
    info[0] = M.cstep; info[1] = M.reach;
    const int Wb = W + 2 * DSDF_BORDER, Hb = H + 2 * DSDF_BORDER;
    for (int py = 0; py < Hb; ++py)
        for (int px = 0; px < Wb; ++px) {
            const size_t i = (size_t)py * Wb + px;
            ref[i] = near[i] = 0;
            if (!list[i]) continue;
            const CamRay r = pixel_centre_ray(*cam, *prm, px, py, W, H);
            const bool hit = (list[i] & 2) != 0;
            Counts a, b, c;
            ref[i] = (unsigned short)fine_proofs<false>(S.G, S.Bc, M.cstep, S.Bmin, S.Bmax, vb, *prm, r.o, r.d, M.fstep, hit, a);
            near[i] = (unsigned short)fine_proofs<true>(S.G, S.Bc, M.cstep, S.Bmin, S.Bmax, vb, *prm, r.o, r.d, M.fstep, hit, b);
            // (the entry without counters is what the kernel calls: it must be the same function)
            if (pixel_fine_proofs_near(S.G, S.Bc, M.cstep, S.Bmin, S.Bmax, vb, *prm, r.o, r.d, M.fstep, hit) != near[i] ||
                pixel_fine_proofs(S.G, S.Bmin, S.Bmax, vb, *prm, r.o, r.d, M.fstep, hit) != ref[i]) return -1.f;
            const ProofRay R = proof_ray(*prm, r.o, r.d);
            float *v = ival + 4 * i;
            v[0] = INFINITY; v[1] = -INFINITY; v[2] = R.t0; v[3] = R.t1;
            if (R.hit) { const ProofInterval I = proof_interval(S.G, S.Bc, R, r.o, r.d, M.cstep, c); v[0] = I.ta; v[1] = I.tb; }
            for (int k = 0; k < DSDF_PC_N; ++k) { cnt[(2 * i) * DSDF_PC_N + k] = a.n[k]; cnt[(2 * i + 1) * DSDF_PC_N + k] = b.n[k]; }
        }
    return M.fstep;
}

// The certificate, position by position, for EVERY film-block pixel whose centre ray meets the box: `wmin` (rz,ry,rx) holds window
// minima the CALLER computed (brute force in the test).  Walks the positions of the fine loop, on its lattice, and returns per pixel
// the smallest wmin among the positions outside [ta, tb] (out_min; +inf: there is none; -inf: the restricted form leaves out a round
// that holds a position INSIDE the interval), their
// number (out_n) and the bound they must exceed (thr = max(thr_hi, 0)).  Returns the step of the fine stages.
float psi_certificate(const float *data, const float *wmin, int rx, int ry, int rz, const dsdf_params *prm, const dsdf_camera *cam, int W,
                      int H, float *out_min, int *out_n, float *thr, float *ival) {
    const ProofMargins M = proof_margins(cam, 1, W, rx, ry, rz);
    if (!(M.fstep > 0.f)) return 0.f;
    const Scene S(data, rx, ry, rz, *prm);
    const BoundGrid Bw = bound_grid(wmin, block_dims(rx, ry, rz, 0), 0, 0.5f);
    const int Wb = W + 2 * DSDF_BORDER, Hb = H + 2 * DSDF_BORDER;
    const float step = M.fstep;
    for (int py = 0; py < Hb; ++py)
        for (int px = 0; px < Wb; ++px) {
            const size_t i = (size_t)py * Wb + px;
            out_min[i] = INFINITY; out_n[i] = 0; thr[i] = 0.f;
            float *v = ival + 4 * i;
            v[0] = v[1] = v[2] = v[3] = 0.f;
            const CamRay r = pixel_centre_ray(*cam, *prm, px, py, W, H);
            const ProofRay R = proof_ray(*prm, r.o, r.d);
            if (!R.hit) continue;
            Counts c;
            const ProofInterval I = proof_interval(S.G, S.Bc, R, r.o, r.d, M.cstep, c);
            v[0] = I.ta; v[1] = I.tb; v[2] = R.t0; v[3] = R.t1;
            thr[i] = fmaxf(R.thr_hi, 0.f);
            const float tend = I.tb < R.t1 ? I.tb : INFINITY;
            for (float tb = R.t0; tb < R.t1 + step; tb += 4.f * step) {
                // a round the restricted form leaves out: all four positions before ta, or the round begins beyond tb
                const bool left_out = I.ta > I.tb || tb + 3.f * step < I.ta || tb > tend;
                for (int k = 0; k < 4; ++k) {
                    if (!(tb + (float)k * step < R.t1 + step)) break;
                    const float tc = fminf(tb + (float)k * step, R.t1);
                    const bool outside = I.ta > I.tb || tc < I.ta || tc > I.tb;
                    if (left_out && !outside) out_min[i] = -INFINITY;          // the form would skip a position it has no certificate for
                    if (!outside) continue;
                    out_min[i] = fminf(out_min[i], bound_at(Bw, S.G, fma3(tc, r.d, r.o)));
                    ++out_n[i];
                }
            }
        }
    return step;
}

}
