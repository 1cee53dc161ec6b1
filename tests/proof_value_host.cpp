// proof_value_host.cpp -- TEST-ONLY stand-alone host build of the THIRD proof stage (csrc/dsdf_proof.h: ValueBound,
// pixel_fine_proofs): the gradient bound built serially, and per listed pixel the merged one-loop form of the second and third
// stage beside the two-loop form of the second (pixel_empty_proof, then pixel_hit_proof).  Compiled by tests/proof_value_cases.py;
// the shared host harness knows nothing of this stage.
#include <algorithm>
#include <vector>
#include "../differentiable-sdf-rendering_amd/csrc/dsdf_lane.h"
#include "../differentiable-sdf-rendering_amd/csrc/dsdf_proof.h"

using namespace dsdf;

static std::vector<float> pad(const float *data, int rx, int ry, int rz) {
    const int sx = rx + 2 * DSDF_APRON, sy = ry + 2 * DSDF_APRON, sz = rz + 2 * DSDF_APRON;
    std::vector<float> out((size_t)sx * sy * sz);
    for (int z = 0; z < sz; ++z)
        for (int y = 0; y < sy; ++y)
            for (int x = 0; x < sx; ++x) {
                const int cx = iclamp(x - DSDF_APRON, 0, rx - 1), cy = iclamp(y - DSDF_APRON, 0, ry - 1), cz = iclamp(z - DSDF_APRON, 0, rz - 1);
                out[((size_t)z * sy + y) * sx + x] = data[((size_t)cz * ry + cy) * rx + cx];
            }
    return out;
}

// Window minima / maxima as the three k_window passes build them: over [i + lo, i + hi] (clamped) along x, then y, then z.
static std::vector<float> window(const float *data, int rx, int ry, int rz, bool maxi) {
    const size_t total = (size_t)rx * ry * rz;
    std::vector<float> a(data, data + total), b(total);
    const int n[3] = {rx, ry, rz};
    const size_t st[3] = {1, (size_t)rx, (size_t)rx * ry};
    for (int ax = 0; ax < 3; ++ax) {
        for (size_t i = 0; i < total; ++i) {
            const int c = (int)((i / st[ax]) % (size_t)n[ax]);
            float m = maxi ? -INFINITY : INFINITY;
            for (int o = DSDF_FINE_LO; o <= DSDF_FINE_HI; ++o) {
                const int q = std::min(std::max(c + o, 0), n[ax] - 1);
                const float v = a[i + (size_t)(q - c) * st[ax]];
                m = maxi ? fmaxf(m, v) : fminf(m, v);
            }
            b[i] = m;
        }
        a.swap(b);
    }
    return a;
}

extern "C" {

// D[0..2]: the largest |difference of adjacent taps| along x, y, z (what k_tap_diff_max leaves on the device).
void pvh_tap_diff_max(const float *data, int rx, int ry, int rz, float *D) {
    D[0] = D[1] = D[2] = 0.f;
    for (int z = 0; z < rz; ++z)
        for (int y = 0; y < ry; ++y)
            for (int x = 0; x < rx; ++x) {
                const size_t i = ((size_t)z * ry + y) * rx + x;
                if (x + 1 < rx) D[0] = fmaxf(D[0], fabsf(data[i + 1] - data[i]));
                if (y + 1 < ry) D[1] = fmaxf(D[1], fabsf(data[i + (size_t)rx] - data[i]));
                if (z + 1 < rz) D[2] = fmaxf(D[2], fabsf(data[i + (size_t)rx * ry] - data[i]));
            }
}

// For every film-block pixel k_pixel_skip would list from the block-bound flags `coarse` (neither bit 0 nor bit 4, or bit 0 without
// bit 1), in the encoding of the flag byte (bit 7 primal-empty, bit 1 gradient-empty, bit 4 hit):
//   two[]    what the second stage ADDS in its two-loop form: pixel_empty_proof over the window minima, then -- where that adds nothing,
//            want_hit, and bit 0 is clear -- pixel_hit_proof over the window maxima;
//   merged[] the same from pixel_fine_proofs' low byte;
//   third[]  what the third stage proves (pixel_fine_proofs' second byte).
// Returns the step of hit_step_fine (0: the stages are off for this film); info[0] = r of the gradient bound, info[1..3] = D.
float pvh_proofs(const float *data, int rx, int ry, int rz, const dsdf_params *prm, const dsdf_camera *cam, int W, int H,
                 const unsigned char *coarse, int want_hit, unsigned char *two, unsigned char *merged, unsigned char *third, float *info) {
    const float fstep = hit_step_fine(cam, 1, W, rx, ry, rz);
    if (!(fstep > 0.f)) return 0.f;
    std::vector<float> p = pad(data, rx, ry, rz);
    GridView G = make_view(p.data(), rx, ry, rz, *prm);
    std::vector<float> fmin = window(data, rx, ry, rz, false), fmax = window(data, rx, ry, rz, true);
    BoundGrid Bmin, Bmax;
    Bmin.b = fmin.data(); Bmin.cx = rx; Bmin.cy = ry; Bmin.cz = rz; Bmin.shift = 0; Bmin.off = 0.5f;
    Bmax = Bmin; Bmax.b = fmax.data();
    float D[3];
    pvh_tap_diff_max(data, rx, ry, rz, D);
    ValueBound vb;
    vb.D = D; vb.r = value_bound_reach(cam, 1, W, rx, ry, rz, fstep);
    info[0] = vb.r; info[1] = D[0]; info[2] = D[1]; info[3] = D[2];
    auto enc = [](unsigned m) { return (unsigned char)(((m & DSDF_PX_EMPTY) ? DSDF_PX_EMPTY_FINE : 0u) | (m & (DSDF_PX_EMPTY_G | DSDF_PX_HIT))); };
    const int Wb = W + 2 * DSDF_BORDER, Hb = H + 2 * DSDF_BORDER;
    for (int py = 0; py < Hb; ++py)
        for (int px = 0; px < Wb; ++px) {
            const size_t i = (size_t)py * Wb + px;
            const unsigned f = coarse[i];
            two[i] = merged[i] = third[i] = 0;
            if (!(!(f & (DSDF_PX_EMPTY | DSDF_PX_HIT)) || (f & 3u) == DSDF_PX_EMPTY)) continue;
            CamRay r = camera_ray(*cam, *prm, (float)(px - DSDF_BORDER) + 0.5f, (float)(py - DSDF_BORDER) + 0.5f, W, H);
            V3 d = r.d * rsqf(dot(r.d, r.d));
            const bool hit = want_hit && !(f & DSDF_PX_EMPTY);
            unsigned m = pixel_empty_proof(G, Bmin, *prm, r.o, d, fstep);
            if (!m && hit) m = pixel_hit_proof(G, Bmax, *prm, r.o, d, fstep);
            two[i] = enc(m);
            const unsigned q = pixel_fine_proofs(G, Bmin, Bmax, vb, *prm, r.o, d, fstep, hit);
            merged[i] = enc(q & 0xffu);
            third[i] = enc(q >> 8);
        }
    return fstep;
}

// Per film sample (lane = pixel * spp + s) of the pixels with mask != 0: bit 0 = the primal's value-only march hits, bit 1 = the
// differentiable march hits, bit 2 = its boundary weight is positive (warp_weight_positive: the statements the gradient sweep runs).
void pvh_trace(const float *data, int rx, int ry, int rz, const dsdf_params *prm, const dsdf_camera *cam, int W, int H, int spp,
               unsigned seed, const unsigned char *mask, unsigned char *out) {
    std::vector<float> p = pad(data, rx, ry, rz);
    GridView G = make_view(p.data(), rx, ry, rz, *prm);
    ViewArgs A;
    A.cam = *cam; A.W = W; A.H = H; A.Wb = W + 2 * DSDF_BORDER; A.Hb = H + 2 * DSDF_BORDER; A.spp = spp;
    A.integrator = DSDF_SILHOUETTE; A.flags = DSDF_REPARAM; A.seed = seed; A.offsets = nullptr; A.emitter_u = nullptr; A.bsdf_u = nullptr;
    const long npix = (long)A.Wb * A.Hb;
    for (long pix = 0; pix < npix; ++pix) {
        if (!mask[pix]) continue;
        for (int s = 0; s < spp; ++s) {
            const long lane = pix * spp + s;
            Lane L = lane_setup(A, *prm, (uint32_t)lane);
            TraceOut tp, t;
            trace_plain(G, *prm, L.ray.o, L.ray.d, L.ray.maxt, tp);
            trace_diff(G, *prm, L.ray.o, L.ray.d, L.ray.maxt, t);
            out[lane] = (unsigned char)((tp.its_t < INFINITY ? 1 : 0) | (t.its_t < INFINITY ? 2 : 0) |
                                        (warp_weight_positive(G, *prm, L.ray.o, L.ray.d, t) ? 4 : 0));
        }
    }
}

}
