// dsdf_proof.h -- per-pixel proofs about what tracing WOULD return (host/device inline; the kernels are in dsdf_skip.h,
// the CPU test-suite checks the same functions against traced rays through tests/harness).  Everything the proofs share is written
// once here: the per-element statements that build the bounds (block_reduce / block_dilate / window_pass / tap_diff_fold: a kernel
// of dsdf_skip.h or a serial loop of a host build decodes an index, calls one and stores), what a proof knows of its ray
// (pixel_centre_ray, ProofRay), the sample logic (HitRun, empty_bits, px_fine_bits), and on the host side the layout of the grid
// buffer (GridLayout) and the margins under which the proofs hold (ProofMargins).
//
// Cubic B-spline weights are >= 0 and sum to 1, so every SDF lookup lies between the minimum and the maximum of its 64 taps.
// Conservative block minima / maxima of the grid, dilated so that they cover every tap of every lookup any SAMPLE ray of a film
// pixel can make near a point of the pixel's CENTRE ray (margins: ProofMargins, below), bound the field along
// all rays of the pixel at once:
//   * empty-space proof  (bits 0 / 1): the lower bound stays above the hit threshold along the whole centre ray -> every
//     sample misses (primal) and has a zero boundary weight (gradient pass);
//     -- in two stages: on the dilated block minima (bits 0 / 1), then, for the pixels those leave, on full-resolution window
//     minima (bits 7 / 1: ProofMargins::fstep, k_pixel_hit_fine).  Bit 0 keeps meaning "proven by the BLOCK minima"; a reader that wants
//     "the primal's samples all miss" asks px_primal_empty;
//     -- and a third stage for both proofs: the spline value on the centre ray -+ a gradient bound (ValueBound, below), whose results
//     go to a library-private effective plane with the same bit meanings, never to the byte a caller can read;
//   * hit proof (bit 4, silhouette primal): see pixel_hit_proof -> every sample HITS.  The silhouette integrator consumes
//     only the hit flag (sdf_silhouette_reparam.py:20-22), so such a pixel needs no march at all.
// Both are proofs, not approximations: a flagged pixel gets exactly the flags tracing would produce
// (tests/test_proof_host.py, tests/test_gpu_parity.py::test_empty_space_skip_is_exact, test_gpu_config_size.py).
#pragma once
#include "dsdf_math.h"

#define DSDF_PX_EMPTY 1u       /* primal: every sample of the pixel misses */
#define DSDF_PX_EMPTY_G 2u     /* gradient pass: ... and has a zero boundary weight */
#define DSDF_PX_FAR 4u         /* (k_skip_dilate) every pixel within +-4 carries bit 0: the samples reach no output */
#define DSDF_PX_FAR_G 8u       /* ... bit 1 */
#define DSDF_PX_HIT 16u        /* every sample of the pixel hits the surface */
#define DSDF_PX_DEEP 32u       /* (k_skip_dilate) every pixel within +-4 carries bit 4: the samples reach only film pixels of value 1 */
#define DSDF_PX_ONE 64u        /* (k_skip_dilate) every pixel within +-2 carries bit 4: this FILM pixel receives hits only */
#define DSDF_PX_EMPTY_FINE 128u /* primal: every sample misses, proven by the second stage on the full-resolution window minima */
#define DSDF_PX_KEEP (DSDF_PX_EMPTY | DSDF_PX_EMPTY_G | DSDF_PX_HIT | DSDF_PX_EMPTY_FINE)

namespace dsdf {

// "Every sample of the pixel's PRIMAL misses": proven by either stage of the empty-space proof.
DSDF_HD bool px_primal_empty(unsigned f) { return (f & (DSDF_PX_EMPTY | DSDF_PX_EMPTY_FINE)) != 0u; }
// "The march of this pixel's samples is known without running it" for the pass that reads the flags: a miss (primal), a miss with a
// zero boundary weight (gradient pass, bit 1 -- which either stage sets).
template <bool DIFF> DSDF_HD bool px_skip_trace(unsigned f) { return DIFF ? (f & DSDF_PX_EMPTY_G) != 0u : px_primal_empty(f); }

// One array of bounds behind the padded grid (GridLayout, below): dilated block bounds of one level, or window bounds.
struct BoundGrid {
    const float *b;          // (cz,cy,cx) dilated block minima (empty-space proof) or maxima (hit proof)
    int cx, cy, cz, shift;   // blocks per axis, log2(voxels per block)
    float off;               // 0: blocks of voxels, index = floor(x * res) >> shift;  0.5: B-spline cells, index = floor(x * res - 0.5)
};

DSDF_HD float bound_at(const BoundGrid &B, const GridView &G, V3 x) {
    int bx = iclamp((int)floorf((x.x - G.tx) * G.frx - B.off) >> B.shift, 0, B.cx - 1);
    int by = iclamp((int)floorf((x.y - G.ty) * G.fry - B.off) >> B.shift, 0, B.cy - 1);
    int bz = iclamp((int)floorf((x.z - G.tz) * G.frz - B.off) >> B.shift, 0, B.cz - 1);
    return B.b[((size_t)bz * B.cy + by) * B.cx + bx];
}

// ---- The bounds, one element each (k_coarse_reduce / k_coarse_dilate / k_window / k_tap_diff_max and the serial host builds).
template <bool MAX> DSDF_HD float bound_fold(float m, float v) { return MAX ? fmaxf(m, v) : fminf(m, v); }
// min (max) of the grid over block (bx, by, bz) of C^3 voxels
template <bool MAX>
DSDF_HD float block_reduce(const float *__restrict__ data, int rx, int ry, int rz, int bx, int by, int bz, int C) {
    float m = MAX ? -INFINITY : INFINITY;
    for (int z = bz * C; z < rz && z < (bz + 1) * C; ++z)
        for (int y = by * C; y < ry && y < (by + 1) * C; ++y)
            for (int x = bx * C; x < rx && x < (bx + 1) * C; ++x) m = bound_fold<MAX>(m, data[((size_t)z * ry + y) * rx + x]);
    return m;
}
// ... of the block values c0 over the blocks within `radius` of (bx, by, bz)
template <bool MAX>
DSDF_HD float block_dilate(const float *__restrict__ c0, int cx, int cy, int cz, int bx, int by, int bz, int radius) {
    float m = MAX ? -INFINITY : INFINITY;
    const int x1 = bx + radius < cx ? bx + radius : cx - 1, y1 = by + radius < cy ? by + radius : cy - 1, z1 = bz + radius < cz ? bz + radius : cz - 1;
    for (int z = bz > radius ? bz - radius : 0; z <= z1; ++z)
        for (int y = by > radius ? by - radius : 0; y <= y1; ++y)
            for (int x = bx > radius ? bx - radius : 0; x <= x1; ++x)
                m = bound_fold<MAX>(m, c0[((size_t)z * cy + y) * cx + x]);
    return m;
}
// One pass of a sliding window along one axis (stride `st` elements, extent n) at element i: over in[clamp(a + lo .. a + hi)].  Three
// passes (x, y, z) build the window maxima of the hit proof and the window minima of the empty-space proof from sdf.data.
template <bool MAX>
DSDF_HD float window_pass(const float *__restrict__ in, size_t i, int n, size_t st, int lo, int hi) {
    const int a = (int)((i / st) % (size_t)n);
    float m = MAX ? -INFINITY : INFINITY;
    for (int o = lo; o <= hi; ++o) {
        const int b = iclamp(a + o, 0, n - 1);
        m = bound_fold<MAX>(m, in[i + (size_t)(b - a) * st]);   // (b - a may be negative: size_t wrap-around adds up correctly)
    }
    return m;
}
// The |differences| of voxel *v to its upper neighbours (hx / hy / hz: it has one; sy, sz: elements per row, per plane) folded into
// the three maxima of the third stage's gradient bound (ValueBound).
DSDF_HD void tap_diff_fold(const float *__restrict__ v, bool hx, bool hy, bool hz, size_t sy, size_t sz, float &mx, float &my, float &mz) {
    if (hx) mx = fmaxf(mx, fabsf(v[1] - v[0]));
    if (hy) my = fmaxf(my, fabsf(v[sy] - v[0]));
    if (hz) mz = fmaxf(mz, fabsf(v[sz] - v[0]));
}

// ---- What every proof knows of its ray.
// The centre ray of film-block pixel (px, py), direction normalised.
DSDF_HD CamRay pixel_centre_ray(const dsdf_camera &cam, const dsdf_params &P, int px, int py, int W, int H) {
    CamRay r = camera_ray(cam, P, (float)(px - DSDF_BORDER) + 0.5f, (float)(py - DSDF_BORDER) + 0.5f, W, H);
    r.d = r.d * rsqf(dot(r.d, r.d));
    return r;
}

// a slightly larger box than the traced one: sample rays may enter where the centre ray does not ...
#define DSDF_PROOF_GROW 0.02f
// ... [t0, t1] of the centre ray in it; [i0, i1] in the traced box SHRUNK by as much (pixel_hit_proof); the two thresholds the
// lower bound has to clear for bit 0 (thr_p) and for bit 1 (thr_hi >= thr_p).
struct ProofRay {
    bool hit, in_hit;          // the ray passes the grown / the shrunk box in front of its origin
    float t0, t1, i0, i1, thr_p, thr_hi;
};
DSDF_HD ProofRay proof_ray(const dsdf_params &P, V3 o, V3 d) {
    const BoxHit b = bbox_ray_intersect(-P.bbox_delta - DSDF_PROOF_GROW, 1.f + P.bbox_delta + DSDF_PROOF_GROW, o, d);
    const BoxHit in = bbox_ray_intersect(-P.bbox_delta + DSDF_PROOF_GROW, 1.f + P.bbox_delta - DSDF_PROOF_GROW, o, d);
    ProofRay R;
    R.hit = b.hit && b.maxt > 0.f; R.in_hit = in.hit && in.maxt > 0.f;
    R.t0 = fmaxf(b.mint, 0.f); R.t1 = b.maxt;
    R.i0 = fmaxf(in.mint, 0.f); R.i1 = in.maxt;
    R.thr_p = 2.f * P.trace_eps * fmaxf(R.t1, 1.f) + 1e-5f;
    const float thr_g = (P.weight_strategy == 6 ? P.edge_eps * (R.t1 + 0.1f) : P.edge_eps) * 1.05f + 1e-4f;
    R.thr_hi = fmaxf(R.thr_p, thr_g);
    return R;
}
// Bits 0 / 1 from the minimum of the lower bound along the ray.
DSDF_HD unsigned empty_bits(float m, float thr_p, float thr_hi) {
    return (m > thr_p ? DSDF_PX_EMPTY : 0u) | (m > thr_hi ? DSDF_PX_EMPTY_G : 0u);
}
// What a FINE stage (second, third) proves, as the flag byte and the effective plane store it: its bit 0 goes to bit 7.
DSDF_HD unsigned px_fine_bits(unsigned m) {
    return ((m & DSDF_PX_EMPTY) ? DSDF_PX_EMPTY_FINE : 0u) | (m & (DSDF_PX_EMPTY_G | DSDF_PX_HIT));
}

// Empty-space proof of one film-block pixel: bits 0 / 1.
DSDF_HD unsigned pixel_empty_proof(const GridView &G, const BoundGrid &B, const dsdf_params &P, V3 o, V3 d, float step) {
    const ProofRay R = proof_ray(P, o, d);
    if (!R.hit) return 0u;
    const float t1 = R.t1;
    float m = INFINITY;
    // (the minimum only falls: once it is at the smaller threshold neither flag can be set any more -- the pixels on the shape leave
    // the loop where their ray comes within the dilation margin of it, the same flags as the full loop)
    // (four samples per round: their loads do not depend on each other, only the decision to go on does)
    for (float tb = R.t0; tb < t1 + step && m > R.thr_p; tb += 4.f * step) {
        float u[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t = tb + (float)k * step;
            u[k] = t < t1 + step ? bound_at(B, G, fma3(fminf(t, t1), d, o)) : INFINITY;
        }
        m = fminf(m, fminf(fminf(u[0], u[1]), fminf(u[2], u[3])));
    }
    return empty_bits(m, R.thr_p, R.thr_hi);
}

// Hit proof of one film-block pixel (bit 4).  The march of SDFBase.ray_intersect_non_diff (shapes.py:290-339; plain_march_*
// in dsdf_math.h) evaluates v at t, reports a hit when v < trace_eps * max(maxt, 1) (> 0) and otherwise advances by |v| = v.
// Let U(t) bound the field from above at parameter t of every sample ray of the pixel (dilated block maxima along the centre
// ray; sample k stands for the parameters within step / 2 of t_k).  If there is a run of samples [ka, kb] with U < 0 --
// a parameter interval [a, b] = [t_ka - step/2, t_kb + step/2] on which EVERY evaluation is a hit -- and no step taken before
// `a` can land beyond `b`  (a step from t lands at t + v <= t + U(t): J = max over k < ka of t_k + step/2 + U_k, and b >= J),
// then the first iterate >= a lies in [a, b] and hits; an earlier hit is a hit as well.  The interval is kept inside the traced
// box shrunk by DSDF_PROOF_GROW, which the centre ray passes while every sample ray (closer than that, checked on the host) is
// still inside the traced box: all of them enter the box before `a` and none has left it at `b` (b <= maxt).
// Margins: 1e-4 on the landing bound covers the rounding of t (|t| < 4: 2e-7 per step) and of the origin offset of the
// perspective rays; the block dilation covers lookup support, lateral deviation and half a step (ProofMargins::hstep).
struct HitRun {         // the state between samples: J, its value when the current run began, "in a run", "proven"
    float J, Jrun;
    bool in_run, done;
};
#define DSDF_HIT_RUN_INIT {-INFINITY, 0.f, false, false}
DSDF_HD void hit_run_step(HitRun &s, float U, float tc, float half, bool inside) {
    if (s.done) return;
    if (U < 0.f && inside) {
        if (!s.in_run) { s.in_run = true; s.Jrun = s.J; }         // (the samples of the run itself take no step: every evaluation hits)
        if (tc + half >= s.Jrun + 1e-4f) { s.done = true; return; }
    } else s.in_run = false;
    s.J = fmaxf(s.J, tc + half + U);
}
DSDF_HD unsigned pixel_hit_proof(const GridView &G, const BoundGrid &B, const dsdf_params &P, V3 o, V3 d, float step) {
    const ProofRay R = proof_ray(P, o, d);
    if (!(P.trace_eps > 0.f && R.hit && R.in_hit)) return 0u;
    const float t1 = R.t1, half = 0.5f * step;
    HitRun h = DSDF_HIT_RUN_INIT;
    // (four samples per round: their bounds are fetched together -- the loads do not depend on each other, the decisions do)
    for (float tb = R.t0; tb < t1 + step && !h.done; tb += 4.f * step) {
        float tc[4], U[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tc[k] = fminf(tb + (float)k * step, t1);
            U[k] = bound_at(B, G, fma3(tc[k], d, o));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!(tb + (float)k * step < t1 + step)) break;
            hit_run_step(h, U[k], tc[k], half, tc[k] - half >= R.i0 && tc[k] + half <= R.i1);
        }
    }
    return h.done ? DSDF_PX_HIT : 0u;
}

// ---- Third stage: the exact spline value on the centre ray, minus / plus a gradient bound.
// Each gradient component of a tricubic B-spline is a convex combination of differences of ADJACENT taps (cubic weights across the
// axis, quadratic B-spline weights along it: all >= 0, sum 1; clamped taps repeat, their differences are 0).  With D_a the largest
// |difference| along axis a (value per voxel) over the whole grid -- tools/sim_gradient_bound.py: a per-block D_a removes 2 % more of
// the primal's lock-step iterations, not worth a lookup -- every y within r voxels of a centre-ray point x has
//     |v(y) - v(x)| <= r |(D_x, D_y, D_z)|_2                                  (mean value theorem + Cauchy-Schwarz)
// and r = lateral deviation + half a step is what the window bounds cover too (ProofMargins::fstep: < 1 voxel).  Where a window bound of
// the second stage fails its threshold, v(x) -+ margin replaces it in the UNCHANGED logic of pixel_empty_proof / pixel_hit_proof:
// the window bound sits 3-5 voxels from the value on the ray, this one 1-1.7.
// fp32 slack, all of it on the safe side:  (i) r carries 0.01 voxel for the rounding of x * res and of x = o + t d (|x| < 4:
// 2.4e-7 * res < 0.01 voxel up to res = 4e4), like the window stage;  (ii) eval_value sums 64 products through three levels of
// four-term fma chains with weights good to a few ulp: |error| < 32 ulp (1.9e-6) of the largest |tap| it reads.  v is a convex
// combination of those 4^3 taps, so it lies between their extremes, and two of them are at most three tap steps apart per axis:
// every |tap| <= |v| + 3 (D_x + D_y + D_z) -- 4e-6 (|v| + 3 |D|_1);  (iii) D and its norm are rounded: (1 + 1e-5).
struct ValueBound {
    const float *D;    // largest |tap difference| along x, y, z (k_tap_diff_max), nullptr: the stage is off
    float r;           // voxels: lateral deviation + half a step + 0.01 (ProofMargins::reach)
};
struct ValueMargin { float L, tap; };      // margin(v) = L + 4e-6 (|v| + tap)
DSDF_HD ValueMargin value_margin(const ValueBound &vb) {
    const float dn = sqrtf(vb.D[0] * vb.D[0] + vb.D[1] * vb.D[1] + vb.D[2] * vb.D[2]);
    ValueMargin m;
    m.L = vb.r * dn * (1.f + 1e-5f);
    m.tap = 3.f * (vb.D[0] + vb.D[1] + vb.D[2]);
    return m;
}

// ---- Where on its centre ray a listed pixel's fine stages have anything to find.
// The fine stages read, at every sample position, the window bounds of the B-spline cell c = floor(X - 0.5) the position X (voxels)
// lies in: taps [c + DSDF_FINE_LO, c + DSDF_FINE_HI] per axis, all of them integers in (X - 3.5, X + 2.5].  The dilated minima of the
// 8^3 level (min_bounds(0): blocks of C = 8 voxels, dilated by one block) bound, at a point Y of block b = floor(Y) >> 3, every tap of
// [8b - 8, 8b + 15], which contains every integer of [Y - C, Y + C - 1].  So a coarse sample at Y whose bound exceeds a threshold
// certifies that the window MINIMUM -- and with it the window maximum and every spline value -- of every position X with
// |X - Y| <= C - 3.5 = 4.5 voxels per axis exceeds it too  (X + 2.5 <= Y + 7, X - 3.5 >= Y - 8;  clamping taps and blocks to the grid
// is monotone, so the containment survives it).  Both X and Y lie ON the centre ray: the statement is about the numbers the fine loop
// would read, so the pixel's lateral deviation does not enter -- the window bounds account for it themselves.  Coarse samples
// ProofMargins::cstep apart (8 voxels of the longest axis), each standing for the parameters within half a step of it, leave
// 4.5 - 4 = 0.5 voxel for the rounding of t, of x = o + t d and of x * res (below 0.01 voxel, as for the fine stages) and for a sample
// position that differs by an ulp between two builds.
// Two walks, forward from t0 and backward from t1, each up to the first sample whose bound is at or below max(thr_hi, 0), give
// [ta, tb]: at every fine position outside it the window minimum exceeds max(thr_hi, 0).  ta > tb: the whole ray is certified.
struct ProofInterval { float ta, tb; };
// What a replay counts per pixel (tools/sim_proof_interval.py through tests/harness); the device passes NoCount, which compiles to nothing.
enum { DSDF_PC_ROUND, DSDF_PC_LIGHT, DSDF_PC_LEAP, DSDF_PC_BMIN, DSDF_PC_BMAX, DSDF_PC_VALUE, DSDF_PC_WALK, DSDF_PC_N };
struct NoCount { DSDF_HD void add(int, int = 1) {} };
template <class Count>
DSDF_HD ProofInterval proof_interval(const GridView &G, const BoundGrid &Bc, const ProofRay &R, V3 o, V3 d, float cstep, Count &cnt) {
    const float len = R.t1 - R.t0, thr = fmaxf(R.thr_hi, 0.f);
    ProofInterval I = {INFINITY, -INFINITY};
    // samples at distance s = 0, cstep, 2 cstep, .. from the walk's end of the ray, up to and including the first at or beyond the
    // other end (clamped onto it): neighbours are at most cstep apart (four per round: the loads do not depend on each other)
#pragma unroll
    for (int back = 0; back < 2; ++back) {
        bool found = false;
        for (float sb = 0.f; sb < len + cstep && !found; sb += 4.f * cstep) {
            float u[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float s = sb + (float)k * cstep;
                const float t = back ? fmaxf(R.t1 - s, R.t0) : fminf(R.t0 + s, R.t1);
                u[k] = s < len + cstep ? bound_at(Bc, G, fma3(t, d, o)) : INFINITY;
                if (s < len + cstep) cnt.add(DSDF_PC_WALK);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (found || u[k] > thr) continue;          // (a NaN stops the walk)
                found = true;
                // the samples before this one cover what lies more than half a step before it
                const float edge = sb + (float)k * cstep - 0.5f * cstep;
                if (back) I.tb = fmaxf(fminf(R.t1 - edge, R.t1), R.t0);
                else I.ta = fminf(fmaxf(R.t0 + edge, R.t0), R.t1);
            }
        }
        if (!found) { I.ta = INFINITY; I.tb = -INFINITY; return I; }      // every sample of one walk clears: so does the whole ray
    }
    return I;
}

// Second and third stage of one listed pixel in ONE loop over the sample positions both proofs share (they start at the same t0 with
// the same step): low byte = what `Bmin.b ? pixel_empty_proof(Bmin) : 0`, and where that is 0 and want_hit, pixel_hit_proof(Bmax)
// return (tests/test_proof_value_host.py compares); bits 8.. = the same with the bounds tightened by the spline value (0 without
// vb.D or without the window minima).  The third stage proves whatever the second proves -- its bounds are never looser, and a run
// of the hit proof can only start earlier with a smaller landing bound -- so the loop ends when the third stage's minimum is at the
// primal threshold and the second stage's hit proof is decided.  The value is evaluated only where the window straddles what it
// has to clear (see the loop).
// NEAR: only the rounds of that loop that hold a position inside [ta, tb] (proof_interval over the 8^3 minima Bc) run in full -- the
// same flags (tests/test_proof_interval_host.py), from the same sample positions: tb advances by the same additions.  At a position
// outside the interval lo > max(thr_hi, 0), so
//   * m2 and m3 stay on the same side of both thresholds, and so do e_alive and the threshold need_e picks;
//   * need_e is false (lo > thr_hi >= thr_p) and need_h is false (lo > 0 >= -mg.L): no value is evaluated, lo3 = lo, hi3 = hi;
//   * hi3 = hi >= lo > 0: no run of the hit proof starts or goes on, and hit_run_step reduces to J = max(J, tc + half + hi).
// Before ta the landing bound J of a LATER run still needs every hi, exactly: a light round loads the window maxima and folds them
// into J (h3 == h2 there); a pixel without the hit proof only advances tb.  Beyond tb no run can start, J is never read again, and
// the loop ends.  Every position before ta is < t1: live and not clamped.
template <bool NEAR, class Count>
DSDF_HD unsigned fine_proofs(const GridView &G, const BoundGrid &Bc, float cstep, const BoundGrid &Bmin, const BoundGrid &Bmax, const ValueBound &vb,
                             const dsdf_params &P, V3 o, V3 d, float step, bool want_hit, Count &cnt) {
    const ProofRay R = proof_ray(P, o, d);
    if (!R.hit) return 0u;
    want_hit = want_hit && P.trace_eps > 0.f && R.in_hit;
    const bool want_empty = Bmin.b != nullptr, third = want_empty && vb.D != nullptr;
    const float t0 = R.t0, t1 = R.t1, i0 = R.i0, i1 = R.i1, half = 0.5f * step, thr_p = R.thr_p, thr_hi = R.thr_hi;
    ValueMargin mg = {0.f, 0.f};
    if (third) mg = value_margin(vb);
    float m2 = INFINITY, m3 = INFINITY;
    HitRun h2 = DSDF_HIT_RUN_INIT, h3 = h2;
    bool e_alive = want_empty;
    float tb = t0, tend = INFINITY;
    if (NEAR) {
        if (!want_empty && !want_hit) return 0u;
        const ProofInterval I = proof_interval(G, Bc, R, o, d, cstep, cnt);
        if (I.ta > I.tb) {        // nothing to find: both minima clear both thresholds, no run starts
            const unsigned f = want_empty ? (DSDF_PX_EMPTY | DSDF_PX_EMPTY_G) : 0u;
            return third ? (f | (f << 8)) : f;
        }
        if (want_hit) {
            for (; tb + 3.f * step < I.ta; tb += 4.f * step) {
                float tc[4], U[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    tc[k] = tb + (float)k * step;
                    U[k] = bound_at(Bmax, G, fma3(tc[k], d, o));
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) h2.J = fmaxf(h2.J, tc[k] + half + U[k]);
                cnt.add(DSDF_PC_LIGHT); cnt.add(DSDF_PC_BMAX, 4);
            }
            h3 = h2;
        } else {
            for (; tb + 3.f * step < I.ta; tb += 4.f * step) cnt.add(DSDF_PC_LEAP);
        }
        if (I.tb < t1) tend = I.tb;        // (tb == t1: the positions beyond t1 are clamped ONTO it, the loop runs to its own end)
    }
    for (; tb < t1 + step && (!NEAR || tb <= tend) && (e_alive || (want_hit && !h2.done)); tb += 4.f * step) {
        float tc[4], lo[4], hi[4], lo3[4], hi3[4];
        const bool v_alive = third && (e_alive || (want_hit && !h3.done));
        const bool fetch_lo = e_alive || v_alive;
        cnt.add(DSDF_PC_ROUND);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool live = tb + (float)k * step < t1 + step;
            tc[k] = fminf(tb + (float)k * step, t1);
            const V3 x = fma3(tc[k], d, o);
            lo3[k] = lo[k] = fetch_lo && live ? bound_at(Bmin, G, x) : INFINITY;
            hi3[k] = hi[k] = want_hit ? bound_at(Bmax, G, x) : INFINITY;
            if (fetch_lo && live) cnt.add(DSDF_PC_BMIN);
            if (want_hit) cnt.add(DSDF_PC_BMAX);
            // (the value can only matter where the window minimum fails the threshold still in play -- the larger one until the
            // gradient flag is lost, then the primal's -- or, for the hit proof, where v + margin < 0 is possible: minimum < -margin
            // under a maximum >= 0)
            const bool need_e = e_alive && lo[k] <= (m3 > thr_hi ? thr_hi : thr_p);
            const bool need_h = want_hit && !h3.done && hi[k] >= 0.f && lo[k] < -mg.L;
            if (v_alive && live && (need_e || need_h)) {
                const float v = eval_value(G, x), m = mg.L + 4e-6f * (fabsf(v) + mg.tap);
                lo3[k] = fmaxf(lo[k], v - m);
                hi3[k] = fminf(hi[k], v + m);
                cnt.add(DSDF_PC_VALUE);
            }
        }
        m2 = fminf(m2, fminf(fminf(lo[0], lo[1]), fminf(lo[2], lo[3])));
        m3 = fminf(m3, fminf(fminf(lo3[0], lo3[1]), fminf(lo3[2], lo3[3])));
        if (want_hit) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!(tb + (float)k * step < t1 + step)) break;
                const bool inside = tc[k] - half >= i0 && tc[k] + half <= i1;
                hit_run_step(h2, hi[k], tc[k], half, inside);
                hit_run_step(h3, hi3[k], tc[k], half, inside);
            }
        }
        e_alive = want_empty && m3 > thr_p;
    }
    unsigned f2 = want_empty ? empty_bits(m2, thr_p, thr_hi) : 0u, f3 = want_empty ? empty_bits(m3, thr_p, thr_hi) : 0u;
    if (!f2 && want_hit && h2.done) f2 = DSDF_PX_HIT;
    if (!f3 && want_hit && h3.done) f3 = DSDF_PX_HIT;
    return third ? (f2 | (f3 << 8)) : f2;
}
// The reference form: every position from box entry to box exit ...
DSDF_HD unsigned pixel_fine_proofs(const GridView &G, const BoundGrid &Bmin, const BoundGrid &Bmax, const ValueBound &vb, const dsdf_params &P,
                                   V3 o, V3 d, float step, bool want_hit) {
    NoCount none;
    return fine_proofs<false>(G, Bmin, 0.f, Bmin, Bmax, vb, P, o, d, step, want_hit, none);
}
// ... and what the device runs: the stretch near the shape.  Bc: the dilated minima of the 8^3 level, cstep: ProofMargins::cstep.
DSDF_HD unsigned pixel_fine_proofs_near(const GridView &G, const BoundGrid &Bc, float cstep, const BoundGrid &Bmin, const BoundGrid &Bmax,
                                        const ValueBound &vb, const dsdf_params &P, V3 o, V3 d, float step, bool want_hit) {
    NoCount none;
    return fine_proofs<true>(G, Bc, cstep, Bmin, Bmax, vb, P, o, d, step, want_hit, none);
}

}  // namespace dsdf

// ---- host side: the layout of the grid buffer and the margins under which the proofs hold (shared with the CPU tests through
// tests/harness)
// the hit proof's maxima: blocks of 2^3 voxels (DSDF_HIT_SHIFT), dilated by DSDF_HIT_RADIUS blocks
#define DSDF_HIT_SHIFT 1
#define DSDF_HIT_RADIUS 2
// The FINE bounds (second stage of both proofs, for the pixels the block bounds leave undecided): per B-spline cell c the
// maximum (hit proof) / minimum (empty-space proof) over the taps [c - 2, c + 3]^3 -- every tap of every lookup within ONE voxel
// of a point of cell c -- at full resolution (window_pass).  A 6^3-voxel window instead of the 10^3 of the block maxima: shapes a few
// voxels thick and pixels close to the silhouette still prove.
#define DSDF_FINE_LO (-2)
#define DSDF_FINE_HI 3

// Blocks of (1 << shift)^3 voxels per axis, and their number (shift 0: the voxels themselves).
struct BlockDims { int cx, cy, cz; size_t cells; };
static BlockDims block_dims(int rx, int ry, int rz, int shift) {
    const int C = 1 << shift;
    BlockDims d;
    d.cx = (rx + C - 1) / C; d.cy = (ry + C - 1) / C; d.cz = (rz + C - 1) / C;
    d.cells = (size_t)d.cx * d.cy * d.cz;
    return d;
}
static dsdf::BoundGrid bound_grid(const float *b, const BlockDims &d, int shift, float off) {
    dsdf::BoundGrid B;
    B.b = b; B.cx = d.cx; B.cy = d.cy; B.cz = d.cz; B.shift = shift; B.off = off;
    return B;
}

// The library's grid buffer (dsdf_pad_grid; the table in include/dsdf.h): the offset, in floats, of each of its arrays.
//   padded | per coarse level: block minima, the same dilated by one block | block maxima, dilated by DSDF_HIT_RADIUS |
//   window maxima | window minima | (to a multiple of 4 floats) row-block copy of the padded grid (dsdf_math.h)
// The undilated (raw) arrays are scratch once the dilation has run; the third stage's gradient bound D[0..2] ALIASES the first three
// floats of the raw block maxima (has_D: there are three) -- the buffer does not grow.  The window passes ping-pong through the
// region of the row-block copy, larger than the grid, before k_tlayout fills it.
struct GridLayout {
    size_t padded;
    size_t min_raw[DSDF_COARSE_LEVELS], min_dil[DSDF_COARSE_LEVELS];
    size_t max_raw, max_dil;
    size_t D;          // == max_raw
    bool has_D;        // a grid of fewer than three such blocks has no third stage
    size_t win_max, win_min;
    size_t rows;       // (16-byte aligned like the padded grid itself: read with 4-byte-aligned 16-byte loads, written as float4)
    size_t total;
};
static GridLayout grid_layout(int rx, int ry, int rz) {
    GridLayout L;
    size_t n = 0;
    L.padded = n; n += (size_t)(rx + 2 * DSDF_APRON) * (ry + 2 * DSDF_APRON) * (rz + 2 * DSDF_APRON);
    for (int l = 0; l < DSDF_COARSE_LEVELS; ++l) {
        const size_t c = block_dims(rx, ry, rz, DSDF_COARSE_SHIFT(l)).cells;
        L.min_raw[l] = n; L.min_dil[l] = n + c; n += 2 * c;
    }
    const size_t hc = block_dims(rx, ry, rz, DSDF_HIT_SHIFT).cells, vox = (size_t)rx * ry * rz;
    L.max_raw = n; L.max_dil = n + hc; n += 2 * hc;
    L.D = L.max_raw; L.has_D = hc >= 3;
    L.win_max = n; L.win_min = n + vox; n += 2 * vox;
    L.rows = (n + 3) & ~(size_t)3;
    L.total = L.rows + dsdf::tlayout_floats(rx, ry, rz);
    return L;
}

// The margins of one view batch.  With `worst` the largest lateral deviation (voxels) of a sample ray from its pixel's centre ray
// inside the box, <= t_far * (0.7072 px * pixel size):
//   level  finest coarse level whose dilation margin (one block) covers worst + lookup support 2.5 voxels + half a step (-1: none,
//          trace every pixel); step: the march step (world units) of the empty-space proof on it; step0: on the next-coarser level,
//          the first, cheaper attempt (0: there is none)
//   hstep  step of the hit proof on the block maxima, 0 when DSDF_HIT_RADIUS blocks of 2^3 voxels do not hold 2.5 voxels + worst +
//          half a step, or the sample rays stray further than DSDF_PROOF_GROW (world units) from the centre ray (pixel_hit_proof's box
//          argument)
//   fstep  step of the fine stages on the window bounds, 0 when worst + half a step exceed their ONE voxel (0.01 voxel of slack on
//          either side for the rounding of x * res), or the box argument fails
//   reach  the r of the third stage's gradient bound (ValueBound, voxels) at fstep: worst + half a step + 0.01 -- at most 1
//   cstep  step of the walks through the 8^3 minima that bracket the fine stages' loop (proof_interval): the dilated bound of a point's
//          block reaches C = 8 voxels below and C - 1 above the point, a fine window 1.5 - DSDF_FINE_LO = 3.5 below and
//          DSDF_FINE_HI - 0.5 = 2.5 above its position, both on the centre ray: half a step + 0.01 <= C - 3.5, capped at one block
struct ProofMargins {
    int level;
    float step0, step, hstep, fstep, reach, cstep;
};
static ProofMargins proof_margins(const dsdf_camera *cams, int nv, int W, int rx, int ry, int rz) {
    const int rmax = rx > ry ? (rx > rz ? rx : rz) : (ry > rz ? ry : rz);
    const int rmin = rx < ry ? (rx < rz ? rx : rz) : (ry < rz ? ry : rz);
    float worst = 0.f;
    for (int i = 0; i < nv; ++i) {
        float dx = cams[i].origin[0] - 0.5f, dy = cams[i].origin[1] - 0.5f, dz = cams[i].origin[2] - 0.5f;
        float t_far = sqrtf(dx * dx + dy * dy + dz * dz) + 1.0f;
        float rho = t_far * 0.7072f * (2.f * cams[i].tan_half_fov / (float)W) * (float)rmax;
        worst = rho > worst ? rho : worst;
    }
    // bounds that reach `reach` voxels beyond the block of the centre-ray point; steps of at most `cap` voxels
    auto block_step = [&](float reach, float cap) {
        float step_vox = 2.f * (reach - 2.5f - worst);
        if (step_vox < 1.f) return 0.f;
        if (step_vox > cap) step_vox = cap;
        return step_vox / (float)rmax;
    };
    auto level_step = [&](int level) { const float C = (float)(1 << DSDF_COARSE_SHIFT(level)); return block_step(C, C); };
    ProofMargins M = {-1, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int level = DSDF_COARSE_LEVELS - 1; level >= 0 && M.level < 0; --level)
        if ((M.step = level_step(level)) > 0.f) M.level = level;
    if (M.level > 0) M.step0 = level_step(M.level - 1);
    if (!(worst / (float)rmin > 0.5f * DSDF_PROOF_GROW)) {
        M.hstep = block_step((float)(DSDF_HIT_RADIUS << DSDF_HIT_SHIFT), 2.f);
        float step_vox = 2.f * (1.f - worst) - 0.02f;
        if (!(step_vox < 0.25f)) M.fstep = (step_vox > 1.f ? 1.f : step_vox) / (float)rmax;
    }
    M.reach = worst + 0.5f * M.fstep * (float)rmax + 0.01f;
    {
        const float C = (float)(1 << DSDF_COARSE_SHIFT(0));
        const float below = C - (1.5f - (float)DSDF_FINE_LO), above = (C - 1.f) - ((float)DSDF_FINE_HI - 0.5f);
        const float step_vox = 2.f * ((below < above ? below : above) - 0.01f);
        M.cstep = (step_vox > C ? C : step_vox) / (float)rmax;
    }
    return M;
}

// One figure of ProofMargins at a time, under the names these had as functions of their own: host builds written against them
// (tests/harness of an earlier tree) keep compiling.  The library reads ProofMargins.
static int skip_level(const dsdf_camera *cams, int nv, int W, int rx, int ry, int rz, float &step) {
    const ProofMargins M = proof_margins(cams, nv, W, rx, ry, rz);
    step = M.step;
    return M.level;
}
static float hit_step(const dsdf_camera *cams, int nv, int W, int rx, int ry, int rz) { return proof_margins(cams, nv, W, rx, ry, rz).hstep; }
static float hit_step_fine(const dsdf_camera *cams, int nv, int W, int rx, int ry, int rz) { return proof_margins(cams, nv, W, rx, ry, rz).fstep; }
static float value_bound_reach(const dsdf_camera *cams, int nv, int W, int rx, int ry, int rz, float) { return proof_margins(cams, nv, W, rx, ry, rz).reach; }
