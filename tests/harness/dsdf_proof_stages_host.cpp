// dsdf_proof_stages_host.cpp -- TEST-ONLY stand-alone host build of the FINE proof stages (csrc/dsdf_proof.h): the bounds built
// serially from the statements the kernels run (block_reduce / block_dilate / window_pass / tap_diff_fold), the second stage of the
// empty-space proof (pixel_empty_proof over the window minima), per listed pixel the merged one-loop form of the second and third
// stage (pixel_fine_proofs) beside the two-loop form of the second (pixel_empty_proof, then pixel_hit_proof), and the traced sample
// rays all of them are checked against.  Compiled by tests/proof_fine_cases.py; tests/harness/dsdf_host_harness.cpp has the block
// stage.
#include <algorithm>
#include <vector>
#include "../../differentiable-sdf-rendering_amd/csrc/dsdf_lane.h"
#include "../../differentiable-sdf-rendering_amd/csrc/dsdf_proof.h"

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

// Window minima / maxima as the three k_window passes build them: along x, then y, then z.
template <bool MAX>
static std::vector<float> window(const float *data, int rx, int ry, int rz) {
    const size_t total = (size_t)rx * ry * rz, st[3] = {1, (size_t)rx, (size_t)rx * ry};
    const int n[3] = {rx, ry, rz};
    std::vector<float> a(data, data + total), b(total);
    for (int ax = 0; ax < 3; ++ax, a.swap(b))
        for (size_t i = 0; i < total; ++i) b[i] = window_pass<MAX>(a.data(), i, n[ax], st[ax], DSDF_FINE_LO, DSDF_FINE_HI);
    return a;
}

template <bool MAX>
static void block_bounds(const float *data, int rx, int ry, int rz, int shift, int radius, float *raw, float *dilated) {
    const BlockDims d = block_dims(rx, ry, rz, shift);
    for (size_t i = 0; i < d.cells; ++i)
        raw[i] = block_reduce<MAX>(data, rx, ry, rz, (int)(i % d.cx), (int)(i / d.cx % d.cy), (int)(i / d.cx / d.cy), 1 << shift);
    for (size_t i = 0; i < d.cells; ++i)
        dilated[i] = block_dilate<MAX>(raw, d.cx, d.cy, d.cz, (int)(i % d.cx), (int)(i / d.cx % d.cy), (int)(i / d.cx / d.cy), radius);
}

extern "C" {

// The window bounds themselves, (rz,ry,rx), and the block bounds of (1 << shift)^3 voxels, raw and dilated by `radius` blocks,
// ceil(r / 2^shift) per axis: the host test checks them against brute force.
void psh_window(const float *data, int rx, int ry, int rz, int maxi, float *out) {
    std::vector<float> m = maxi ? window<true>(data, rx, ry, rz) : window<false>(data, rx, ry, rz);
    std::copy(m.begin(), m.end(), out);
}
void psh_block_bounds(const float *data, int rx, int ry, int rz, int shift, int radius, int maxi, float *raw, float *dilated) {
    if (maxi) block_bounds<true>(data, rx, ry, rz, shift, radius, raw, dilated);
    else block_bounds<false>(data, rx, ry, rz, shift, radius, raw, dilated);
}

// D[0..2]: the largest |difference of adjacent taps| along x, y, z (what k_tap_diff_max leaves on the device).
void psh_tap_diff_max(const float *data, int rx, int ry, int rz, float *D) {
    D[0] = D[1] = D[2] = 0.f;
    for (int z = 0; z < rz; ++z)
        for (int y = 0; y < ry; ++y)
            for (int x = 0; x < rx; ++x)
                tap_diff_fold(data + ((size_t)z * ry + y) * rx + x, x + 1 < rx, y + 1 < ry, z + 1 < rz, (size_t)rx, (size_t)rx * ry, D[0], D[1], D[2]);
}

// flags (H+4) x (W+4): what pixel_empty_proof returns over the window minima with the step of the fine stages, bits 0 / 1 as that
// function names them (the library stores bit 0 of this stage as bit 7).  Returns the step, 0 = the stage is off for this film.
float psh_fine_empty(const float *data, int rx, int ry, int rz, const dsdf_params *prm, const dsdf_camera *cam, int W, int H,
                     unsigned char *flags) {
    const float fstep = proof_margins(cam, 1, W, rx, ry, rz).fstep;
    if (!(fstep > 0.f)) return 0.f;
    std::vector<float> p = pad(data, rx, ry, rz), fine = window<false>(data, rx, ry, rz);
    const GridView G = make_view(p.data(), rx, ry, rz, *prm);
    const BoundGrid B = bound_grid(fine.data(), block_dims(rx, ry, rz, 0), 0, 0.5f);
    const int Wb = W + 2 * DSDF_BORDER, Hb = H + 2 * DSDF_BORDER;
    for (int py = 0; py < Hb; ++py)
        for (int px = 0; px < Wb; ++px) {
            const CamRay r = pixel_centre_ray(*cam, *prm, px, py, W, H);
            flags[(size_t)py * Wb + px] = (unsigned char)pixel_empty_proof(G, B, *prm, r.o, r.d, fstep);
        }
    return fstep;
}

// For every film-block pixel k_pixel_skip would list from the block-bound flags `coarse` (neither bit 0 nor bit 4, or bit 0 without
// bit 1), in the encoding of the flag byte (px_fine_bits: bit 7 primal-empty, bit 1 gradient-empty, bit 4 hit):
//   two[]    what the second stage ADDS in its two-loop form: pixel_empty_proof over the window minima, then -- where that adds nothing,
//            want_hit, and bit 0 is clear -- pixel_hit_proof over the window maxima;
//   merged[] the same from pixel_fine_proofs' low byte;
//   third[]  what the third stage proves (pixel_fine_proofs' second byte).
// Returns the step of the fine stages (0: they are off for this film); info[0] = r of the gradient bound, info[1..3] = D.
float psh_proofs(const float *data, int rx, int ry, int rz, const dsdf_params *prm, const dsdf_camera *cam, int W, int H,
                 const unsigned char *coarse, int want_hit, unsigned char *two, unsigned char *merged, unsigned char *third, float *info) {
    const ProofMargins M = proof_margins(cam, 1, W, rx, ry, rz);
    const float fstep = M.fstep;
    if (!(fstep > 0.f)) return 0.f;
    std::vector<float> p = pad(data, rx, ry, rz), fmin = window<false>(data, rx, ry, rz), fmax = window<true>(data, rx, ry, rz);
    const GridView G = make_view(p.data(), rx, ry, rz, *prm);
    const BoundGrid Bmin = bound_grid(fmin.data(), block_dims(rx, ry, rz, 0), 0, 0.5f), Bmax = bound_grid(fmax.data(), block_dims(rx, ry, rz, 0), 0, 0.5f);
    float D[3];
    psh_tap_diff_max(data, rx, ry, rz, D);
    const ValueBound vb = {D, M.reach};
    info[0] = vb.r; info[1] = D[0]; info[2] = D[1]; info[3] = D[2];
    const int Wb = W + 2 * DSDF_BORDER, Hb = H + 2 * DSDF_BORDER;
    for (int py = 0; py < Hb; ++py)
        for (int px = 0; px < Wb; ++px) {
            const size_t i = (size_t)py * Wb + px;
            const unsigned f = coarse[i];
            two[i] = merged[i] = third[i] = 0;
            if (!(!(f & (DSDF_PX_EMPTY | DSDF_PX_HIT)) || (f & 3u) == DSDF_PX_EMPTY)) continue;
            const CamRay r = pixel_centre_ray(*cam, *prm, px, py, W, H);
            const bool hit = want_hit && !(f & DSDF_PX_EMPTY);
            unsigned m = pixel_empty_proof(G, Bmin, *prm, r.o, r.d, fstep);
            if (!m && hit) m = pixel_hit_proof(G, Bmax, *prm, r.o, r.d, fstep);
            two[i] = (unsigned char)px_fine_bits(m);
            const unsigned q = pixel_fine_proofs(G, Bmin, Bmax, vb, *prm, r.o, r.d, fstep, hit);
            merged[i] = (unsigned char)px_fine_bits(q & 0xffu);
            third[i] = (unsigned char)px_fine_bits(q >> 8);
        }
    return fstep;
}

// Per film sample (lane = pixel * spp + s) of the pixels with mask != 0: bit 0 = the primal's value-only march hits, bit 1 = the
// differentiable march hits, bit 2 = its boundary weight is positive (warp_weight_positive: 1 - |v(x_warp)| / min(edge_eps * warp_t, bd)
// > 0 with a positive weight sum -- the statements the gradient sweep runs).
void psh_trace(const float *data, int rx, int ry, int rz, const dsdf_params *prm, const dsdf_camera *cam, int W, int H, int spp,
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
