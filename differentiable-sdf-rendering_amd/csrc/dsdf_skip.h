// dsdf_skip.h -- the kernels of the per-pixel proofs (included by dsdf_kernels.hip): those that build the bounds behind the padded
// grid, the proof kernels themselves, the dilation of their flags over the film, and the host-side views of the grid buffer
// (GridLayout, dsdf_proof.h).  What a kernel computes per element is a statement of dsdf_proof.h, shared with the serial host builds
// of the CPU tests: a kernel here decodes its index, calls it and stores.
#pragma once

// ------------------------------------------------------------------ the bounds (dsdf_proof.h)
// `c0[b]` = min (max) of the grid over coarse block b; `c[b]` = the same over the blocks within `radius` of b.  The
// empty-space proof uses minima over 8^3 or 4^3 voxels dilated by one block (the finest level whose margin covers the pixel
// footprint); the hit proof maxima over 2^3 voxels dilated by two blocks (a 10^3-voxel window: tighter, so that thin parts of
// the shape still prove).
template <bool MAX>
__global__ void k_coarse_reduce(const float *__restrict__ data, int rx, int ry, int rz, float *__restrict__ c0, int cx, int cy, int cz,
                                int C) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cx * cy * cz) return;
    c0[i] = block_reduce<MAX>(data, rx, ry, rz, i % cx, (i / cx) % cy, i / (cx * cy), C);
}

template <bool MAX>
__global__ void k_coarse_dilate(const float *__restrict__ c0, float *__restrict__ c, int cx, int cy, int cz, int radius) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cx * cy * cz) return;
    c[i] = block_dilate<MAX>(c0, cx, cy, cz, i % cx, (i / cx) % cy, i / (cx * cy), radius);
}

template <bool MAX>
__global__ void k_window(const float *__restrict__ in, float *__restrict__ out, size_t total, int n, size_t st, int lo, int hi) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) out[i] = window_pass<MAX>(in, i, n, st, lo, hi);
}

// The gradient bound of the third proof stage (dsdf_proof.h: ValueBound): D[a] = the largest |difference of adjacent taps| along x, y, z
// over the whole grid.  D is zeroed by the caller; non-negative floats order like their bit patterns, so the maximum is an integer one.
__global__ __launch_bounds__(256) void k_tap_diff_max(const float *__restrict__ data, int rx, int ry, int rz, int *__restrict__ D) {
    float mx = 0.f, my = 0.f, mz = 0.f;
    // (one row of x per block and turn: no 64-bit division per voxel)
    for (int row = blockIdx.x; row < ry * rz; row += gridDim.x) {
        const int y = row % ry, z = row / ry;
        const float *r = data + (size_t)row * rx;
        for (int x = threadIdx.x; x < rx; x += blockDim.x)
            tap_diff_fold(r + x, x + 1 < rx, y + 1 < ry, z + 1 < rz, (size_t)rx, (size_t)rx * ry, mx, my, mz);
    }
    // (thousands of atomics on three addresses would cost more than the pass over the grid: one wave per block reduces the block's
    // maxima and issues an atomic only for a value above what is stored -- D only grows)
    __shared__ int part[4][3];
    const int ix = wave_max_i32(__float_as_int(mx)), iy = wave_max_i32(__float_as_int(my)), iz = wave_max_i32(__float_as_int(mz));
    if (lane_id() == 0) { part[threadIdx.x >> 6][0] = ix; part[threadIdx.x >> 6][1] = iy; part[threadIdx.x >> 6][2] = iz; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int m = max(max(part[0][threadIdx.x], part[1][threadIdx.x]), max(part[2][threadIdx.x], part[3][threadIdx.x]));
        if (m > __atomic_load_n(D + threadIdx.x, __ATOMIC_RELAXED)) atomicMax(D + threadIdx.x, m);
    }
}

// flags[view][Hb*Wb]: DSDF_PX_EMPTY / _EMPTY_G / _HIT of every film-block pixel (dsdf_proof.h).  step == 0: no empty-space
// proof, hstep == 0: no hit proof (margins not covered, or the integrator consumes more than the hit flag).
// `plane` (optional): the effective plane of the third stage (k_skip_dilate), cleared here.
// `undecided` (optional): [0] = counter (zeroed by the caller), entries from [DSDF_UNDECIDED_HDR]: view * Wb * Hb + pixel of every
// pixel neither proof settled -- the work list of k_pixel_hit_fine -- and, with list_g (a gradient pass will read these flags and
// the fine empty-space stage runs), of every pixel with bit 0 but not bit 1: the fine minima may still give it bit 1.
#define DSDF_UNDECIDED_HDR 16
// step0 > 0: a first, cheaper attempt at the empty-space proof on the next-coarser level Bmin0 (blocks twice as large, steps twice
// as long): most pixels of a silhouette view pass far from the shape and are settled there.
__global__ void k_pixel_skip(GridView G, BoundGrid Bmin0, BoundGrid Bmin, BoundGrid Bmax, dsdf_params P, ViewBatch VB,
                             unsigned char *__restrict__ flags, float step0, float step, float hstep, uint32_t *__restrict__ undecided,
                             int list_g, unsigned char *__restrict__ plane) {
    const ViewArgs &A = VB.v[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x, npix = A.Wb * A.Hb;
    const bool valid = i < npix;
    unsigned f = DSDF_PX_EMPTY;
    if (valid) {
        int py = i / A.Wb, px = i - py * A.Wb;
        const CamRay r = pixel_centre_ray(A.cam, P, px, py, A.W, A.H);
        if (step0 > 0.f) f = pixel_empty_proof(G, Bmin0, P, r.o, r.d, step0);
        else f = 0u;
        if (f != (DSDF_PX_EMPTY | DSDF_PX_EMPTY_G) && step > 0.f) f |= pixel_empty_proof(G, Bmin, P, r.o, r.d, step);
        if (hstep > 0.f && !(f & DSDF_PX_EMPTY)) f |= pixel_hit_proof(G, Bmax, P, r.o, r.d, hstep);
        flags[(size_t)blockIdx.y * npix + i] = (unsigned char)f;
        if (plane) plane[(size_t)blockIdx.y * npix + i] = 0;         // (k_pixel_hit_fine adds what the third stage proves)
    }
    if (undecided) {
        const bool open = valid && (!(f & (DSDF_PX_EMPTY | DSDF_PX_HIT)) || (list_g && (f & 3u) == DSDF_PX_EMPTY));
        const uint64_t m = __ballot(open);
        if (m != 0) {
            const int leader = __builtin_ctzll(m);
            uint32_t base = 0;
            if (lane_id() == leader) base = atomicAdd(undecided, (uint32_t)__popcll(m));
            base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
            if (open) undecided[DSDF_UNDECIDED_HDR + base + mask_prefix(m)] = (uint32_t)blockIdx.y * (uint32_t)npix + (uint32_t)i;
        }
    }
}

// Second stage of both proofs on the pixels k_pixel_skip listed.  First the empty-space proof, pixel_empty_proof itself over the
// full-resolution window MINIMA (Bmin.b != nullptr: DSDF_NO_FINE_EMPTY switches the stage off): the block minima only prove a pixel whose rays stay 6-8 voxels clear of the
// surface, these one whose rays stay about 3.  Its result goes to bit 7 (DSDF_PX_EMPTY_FINE) and bit 1, never to bit 0, which
// keeps meaning "proven by the block minima".  Then, where that fails and the hit proof is wanted (hit), on the pixels without
// bit 0, pixel_hit_proof (dsdf_proof.h) over the window maxima -- ~600 samples half a voxel apart per ray.  Inside k_pixel_skip that loop cost 1.2 ms per
// 12-view step: a few undecided pixels per wave, each a serial chain on an otherwise idle wave; a wave-cooperative form (64
// samples of one pixel per wave iteration, prefix maxima by shuffles) did MORE work, 1.7 ms.  So the undecided pixels are
// COMPACTED (k_pixel_skip appends them to a list, one reservation per wave) and a dense launch runs the serial form, one pixel
// per lane, every wave full.
// Third stage (vb.D != nullptr, plane != nullptr), in the same loop: where a window bound fails, the spline value on the centre ray
// -+ a gradient bound (dsdf_proof.h: ValueBound).  What it proves beyond the second stage goes to `plane`, the library-private
// effective plane, with the same bit meanings (7 / 1 / 4); `flags`, which a caller may read, is written byte for byte as without it.
// (As a launch of its own over the pixels the second stage leaves it cost 1.0 + 1.6 ms per proof instead of 1.9: DESIGN 5.61.)
// The loop runs only over the stretch of the centre ray near the shape (dsdf_proof.h: proof_interval -- two short walks through the
// dilated 8^3 minima Bc, cstep apart, in this kernel's preamble), with the flags of the whole ray.
__global__ __launch_bounds__(256) void k_pixel_hit_fine(GridView G, BoundGrid Bc, float cstep, BoundGrid Bmin, BoundGrid B, ValueBound vb, dsdf_params P, ViewBatch VB,
                                                        unsigned char *__restrict__ flags, unsigned char *__restrict__ plane,
                                                        const uint32_t *__restrict__ count, const uint32_t *__restrict__ list, float step,
                                                        int hit) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *count) return;
    const uint32_t e = list[i], npix = (uint32_t)(VB.v[0].Wb * VB.v[0].Hb), view = e / npix, pix = e - view * npix;
    const ViewArgs &A = VB.v[view];
    const int py = (int)(pix / (uint32_t)A.Wb), px = (int)(pix - (uint32_t)py * (uint32_t)A.Wb);
    const CamRay r = pixel_centre_ray(A.cam, P, px, py, A.W, A.H);
    const unsigned f = flags[e];
    // both stages, both proofs, one loop over the sample positions (dsdf_proof.h); the hit proof only for the pixels without bit 0
    const unsigned m = pixel_fine_proofs_near(G, Bc, cstep, Bmin, B, vb, P, r.o, r.d, step, hit && !(f & DSDF_PX_EMPTY));
    const unsigned add = px_fine_bits(m & 0xffu), add3 = px_fine_bits(m >> 8);
    if (add) flags[e] = (unsigned char)(f | add);
    // the third stage's results never reach the caller-visible byte: the render stages read them from the effective plane
    if (plane && add3) plane[e] = (unsigned char)add3;
}

// Bits 2/3 (DSDF_PX_FAR / _FAR_G): every film pixel within +-4 of this one carries bit 0 or 7 (px_primal_empty) / bit 1.  A sample only splats into
// pixels within +-2 of its own, and a film pixel's weight sum only matters if a value lands on it or a
// backward lane reads its adjoint -- both need a pixel within +-2 of it that is NOT proven empty.  So the
// samples of a pixel with bit 2 (3) set cannot influence any output of the primal (gradient) pass and are
// not generated at all.  (In place: writers only add bits 2/3, readers only look at bits 0/1.)
#define DSDF_FAR_RADIUS 4
// Bits 5/6 (DSDF_PX_DEEP / _ONE), the same argument for the hit proof of the silhouette primal: a film pixel all of whose
// contributors (the pixels within +-2) carry DSDF_PX_HIT receives only samples of value 1, so its value channel EQUALS its
// weight channel and it develops to 1 whatever the samples are (bit 6); a pixel whose whole +-4 neighbourhood carries
// DSDF_PX_HIT only ever feeds such film pixels, so its samples are not generated (bit 5) -- k_film_ones adds (1, 1) to every
// bit-6 film pixel instead, which leaves value == weight where samples still arrive and gives 1 / 1 where none does.
// `plane` (optional, the third stage's effective plane): holds the KEEP bits the third stage ADDS (k_pixel_hit_fine); this pass completes
// it to what the render stages read -- the KEEP bits of flags | plane and bits 2 / 3 / 5 / 6 recomputed from those -- in the same
// sweep over the neighbourhood.  In place like `flags`: a neighbour already rewritten holds flags' KEEP bits too, the same union.
struct FarAcc {       // AND of bits 0 / 1 / 4 over the pixels within +-4 (bit 0: proven empty by either stage), of bit 4 over those within +-2
    unsigned m = 3u | DSDF_PX_HIT, near = DSDF_PX_HIT;
    __device__ void add(unsigned v, bool close) {
        m &= v | (px_primal_empty(v) ? DSDF_PX_EMPTY : 0u);
        if (close) near &= v;
    }
    // the stored byte: the pixel's own KEEP bits, bits 2 / 3 / 5 / 6 from the neighbourhood
    __device__ unsigned char byte(unsigned own) const {
        return (unsigned char)((own & DSDF_PX_KEEP) | ((m & 3u) << 2) | ((m & DSDF_PX_HIT) ? DSDF_PX_DEEP : 0u) | (near ? DSDF_PX_ONE : 0u));
    }
};
__global__ void k_skip_dilate(ViewBatch VB, unsigned char *__restrict__ flags, unsigned char *__restrict__ plane) {
    const ViewArgs &A = VB.v[blockIdx.y];
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.Wb * A.Hb) return;
    unsigned char *f = flags + (size_t)blockIdx.y * A.Wb * A.Hb;
    unsigned char *p = plane ? plane + (size_t)blockIdx.y * A.Wb * A.Hb : nullptr;
    int py = i / A.Wb, px = i - py * A.Wb;
    FarAcc af, ap;          // of the flag byte, of flags | plane
    for (int y = max(py - DSDF_FAR_RADIUS, 0); y <= min(py + DSDF_FAR_RADIUS, A.Hb - 1); ++y)
        for (int x = max(px - DSDF_FAR_RADIUS, 0); x <= min(px + DSDF_FAR_RADIUS, A.Wb - 1); ++x) {
            const unsigned v = f[y * A.Wb + x];
            const bool close = abs(y - py) <= 2 && abs(x - px) <= 2;
            af.add(v, close);
            if (p) ap.add(v | (p[y * A.Wb + x] & DSDF_PX_KEEP), close);
        }
    const unsigned own = f[i];
    f[i] = af.byte(own);
    if (p) p[i] = ap.byte(own | p[i]);
}

// sdf_direct_reparam with a VISIBLE environment (round 6): a sample that misses carries the environment's radiance, so "far" pixels
// used to be sampled all the same (82 % of the chunks of the C5 workload: sampler, camera ray, a 4-channel film reduce each).  But a
// film pixel ALL of whose contributors (the pixels within +-2) are proven empty receives only samples of value `env`: it develops to
// env whatever their weights are.  k_film_env adds (env, 1) to every such film pixel of the call's row window; the samples of a far
// pixel (bit 2 / 3: everything within +-4 proven empty) only ever reach such film pixels and are not generated.  Where samples of
// near pixels still arrive, (env + sum w env) / (1 + sum w) = env.  pass_mask: a contributor counts as proven empty when it carries
// one of these bits -- DSDF_PX_EMPTY | DSDF_PX_EMPTY_FINE (primal) or DSDF_PX_EMPTY_G (gradient pass: its film is developed too, and
// no backward lane reads the adjoint of such a pixel).
__global__ void k_film_env(ViewBatch VB, const unsigned char *__restrict__ flags, float *__restrict__ blocks, int row0, int row1,
                           unsigned pass_mask, float er, float eg, float eb) {
    const ViewArgs &A = VB.v[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x, npix = A.Wb * A.Hb;
    if (i >= npix) return;
    const int py = i / A.Wb, px = i - py * A.Wb;
    if (py < row0 || py >= row1) return;
    const unsigned char *f = flags + (size_t)blockIdx.y * npix;
    bool m = true;
    for (int y = max(py - 2, 0); y <= min(py + 2, A.Hb - 1); ++y)
        for (int x = max(px - 2, 0); x <= min(px + 2, A.Wb - 1); ++x) m = m && (f[y * A.Wb + x] & pass_mask) != 0u;
    if (!m) return;
    float *b = blocks + ((size_t)blockIdx.y * npix + i) * 4;
    atomicAdd(b, er); atomicAdd(b + 1, eg); atomicAdd(b + 2, eb); atomicAdd(b + 3, 1.f);
}

// (1, 1) for the film pixels of the call's row window that receive hits only (bit 6): see k_skip_dilate.  The samples of the
// deep pixels (bit 5) are proven hits that nobody generates: the caller's statistics count them as hits all the same.
__global__ void k_film_ones(ViewBatch VB, const unsigned char *__restrict__ flags, float *__restrict__ blocks, int row0, int row1,
                            unsigned long long *stats) {
    const ViewArgs &A = VB.v[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x, npix = A.Wb * A.Hb;
    const int py = i < npix ? i / A.Wb : -1;
    const unsigned f = (py >= row0 && py < row1) ? flags[(size_t)blockIdx.y * npix + i] : 0u;
    if (f & DSDF_PX_ONE) {
        float *b = blocks + ((size_t)blockIdx.y * npix + i) * 2;
        atomicAdd(b, 1.f);
        atomicAdd(b + 1, 1.f);
    }
    if (stats) {
        const int n = wave_sum_i32((f & DSDF_PX_DEEP) ? A.spp : 0);
        if (n && lane_id() == 0) atomicAdd(stats + (size_t)(blockIdx.x & 63u) * DSDF_STAT_SLOTS + 3, (unsigned long long)n);
    }
}

// ---- host side: views of the grid buffer (GridLayout, dsdf_proof.h)
static GridView device_view(const float *padded, int rx, int ry, int rz, const dsdf_params &prm) {
    GridView G = make_view(padded, rx, ry, rz, prm);
    G.pt = padded + grid_layout(rx, ry, rz).rows;
    return G;
}
// the dilated block minima of one coarse level, the dilated block maxima, the window maxima, the window minima
static BoundGrid min_bounds(const float *padded, int rx, int ry, int rz, int level) {
    return bound_grid(padded + grid_layout(rx, ry, rz).min_dil[level], block_dims(rx, ry, rz, DSDF_COARSE_SHIFT(level)), DSDF_COARSE_SHIFT(level), 0.f);
}
static BoundGrid max_bounds(const float *padded, int rx, int ry, int rz) {
    return bound_grid(padded + grid_layout(rx, ry, rz).max_dil, block_dims(rx, ry, rz, DSDF_HIT_SHIFT), DSDF_HIT_SHIFT, 0.f);
}
static BoundGrid fine_bounds(const float *padded, int rx, int ry, int rz) {
    return bound_grid(padded + grid_layout(rx, ry, rz).win_max, block_dims(rx, ry, rz, 0), 0, 0.5f);
}
static BoundGrid fine_min_bounds(const float *padded, int rx, int ry, int rz) {
    return bound_grid(padded + grid_layout(rx, ry, rz).win_min, block_dims(rx, ry, rz, 0), 0, 0.5f);
}
// The third stage's gradient bound D[0..2] (k_tap_diff_max), nullptr: the grid has none, no third stage.
static float *grad_bound(const float *padded, int rx, int ry, int rz) {
    const GridLayout L = grid_layout(rx, ry, rz);
    return L.has_D ? const_cast<float *>(padded) + L.D : nullptr;
}
