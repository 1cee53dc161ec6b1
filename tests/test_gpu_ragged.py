"""GPU parity on RAGGED grid shapes (tests/cases.py RAGGED: x sides at every residue mod 4, y / z sides that are not multiples of the
8^3 / 4^3 / 2^3 proof blocks, a grid thinner than one block, surface up to the +x / +y faces) and ragged films, on the paths of
spp % 64 == 0: the persistent work-list workers, the wave cell cache, the empty-space and hit proofs, the tail hand-off, the wavefront
sdf_direct_reparam with and without the shadow rays' cell table.  Their index arithmetic depends on the grid's shape (the row-block
copy's strides tz4 = 32 (ry + 6), tx4 = tz4 (rz + 6) and its 4-tap x chunks; partial last proof blocks; the cell table's sx / sz), and
the cubic grids of the other parity tests (rx % 4 == 0, sides multiples of 8, rx == rz) cannot see a wrong one.

Every reference is the fp64 C oracle (tests/precision.py, one view at a time); gates are the suite's: images rel-L2 < 1e-4 per view,
gradients max(2 x measured fp32 floor, 1e-4), lookups / traces 2 x the fp32 C build's own error (floored like test_gpu_parity.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import c_oracle
import precision as P
import sdf_oracle as O
from cases import RAGGED, ragged_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD_TOL = 1e-4
NAMES = list(RAGGED)


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    assert torch.cuda.is_available()
    return m


def _grid(dsdf, case):
    return dsdf.SdfGrid(case['grid'].float().cuda())


def _sensors(dsdf, case, views=None):
    cams = dsdf.get_regular_cameras(case['ncam'], resx=case['W'], resy=case['H'])
    return [cams[v['icam']] for v in (views or case['views'])]


# ------------------------------------------------------------------ lookups and traces
def _lookup_points(shape, seed):
    """(x, y, z) points: uniform in [-0.05, 1.05]^3; packed into the first two and the last two cells (and the clamped apron) of
    each axis; exactly on cell boundaries (x r - 0.5 integer) on one axis and on all three."""
    rz, ry, rx = shape
    rng = np.random.default_rng(seed)
    res = np.array([rx, ry, rz], np.float64)
    parts = [rng.uniform(-0.05, 1.05, (20000, 3))]
    for ax in range(3):
        for lo, hi in ((-1.0, 2.0), (res[ax] - 2.0, res[ax] + 1.0)):                  # in voxels
            p = rng.uniform(0.0, 1.0, (2000, 3))
            p[:, ax] = rng.uniform(lo, hi, 2000) / res[ax]
            parts.append(p)
        p = rng.uniform(0.0, 1.0, (2000, 3))
        p[:, ax] = (rng.integers(-1, int(res[ax]) + 1, 2000) + 0.5) / res[ax]
        parts.append(p)
    parts.append((rng.integers(-1, res.astype(int) + 1, (3000, 3)) + 0.5) / res)
    return np.concatenate(parts).astype(np.float32)


@pytest.mark.parametrize('name', NAMES)
def test_eval_cubic_ragged(dsdf, name):
    """dsdf.eval_cubic (orders 0 and 2) against the fp64 C oracle: rel-L2 AND the largest per-point error relative to the value
    range of the grid (for v) / the largest reference magnitude (for g, H) -- a wrong last x chunk is a few % of uniform points."""
    case = ragged_case(name)
    g32 = case['grid'].float().numpy()
    pts = _lookup_points(g32.shape, RAGGED[name][-1])
    vo, go, Ho = c_oracle.eval_cubic(P.clib(True), g32, pts)
    v32, g32o, H32 = c_oracle.eval_cubic(P.clib(False), g32, pts)
    grid = _grid(dsdf, case)
    v, g, H = (t.cpu().numpy() for t in dsdf.eval_cubic(grid, torch.from_numpy(pts).cuda(), 2))
    v0 = dsdf.eval_cubic(grid, torch.from_numpy(pts).cuda(), 0)[0].cpu().numpy()
    scale = dict(v=float(g32.max() - g32.min()), g=float(np.abs(go).max()), H=float(np.abs(Ho).max()))
    bad = []
    for k, out, out32, ref, l2 in (('v', v, v32, vo, 1e-6), ('v0', v0, v32, vo, 1e-6), ('g', g, g32o, go, 1e-5), ('H', H, H32, Ho, 1e-5)):
        s = scale[k[0]]
        e, f = P.rel_l2(out, ref), P.rel_l2(out32, ref)
        m, fm = float(np.abs(out - ref).max()) / s, float(np.abs(out32 - ref).max()) / s
        tol, tolm = max(2 * f, l2), max(2 * fm, l2)
        P.record('eval_cubic_ragged', case=name, output=k, err=e, floor=f, tol=tol, err_max=m, floor_max=fm, tol_max=tolm)
        if not (e <= tol and m <= tolm):
            worst = int(np.abs(out - ref).reshape(len(pts), -1).max(-1).argmax())
            bad.append((k, e, tol, m, tolm, pts[worst].tolist()))
    assert not bad, bad


def _grazing_rays(shape, seed, n=3000):
    """Rays along z that graze the +x face (x within 3 voxels of it, inside and just outside) and rays along x that graze the +y
    face, slightly tilted: they cross the cells of the last x chunk / the last y rows over the whole depth of the grid."""
    rz, ry, rx = shape
    rng = np.random.default_rng(seed)
    o = np.zeros((2 * n, 3)); d = np.zeros((2 * n, 3))
    o[:n, 0] = 1.0 - rng.uniform(-0.5, 3.0, n) / rx
    o[:n, 1] = rng.uniform(0.0, 1.0, n)
    o[:n, 2] = -0.5
    d[:n] = np.stack([rng.normal(0, 0.01, n), rng.normal(0, 0.05, n), np.ones(n)], -1)
    o[n:, 1] = 1.0 - rng.uniform(-0.5, 3.0, n) / ry
    o[n:, 2] = rng.uniform(0.0, 1.0, n)
    o[n:, 0] = -0.5
    d[n:] = np.stack([np.ones(n), rng.normal(0, 0.01, n), rng.normal(0, 0.05, n)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32), np.full(2 * n, 10.0, np.float32)


@pytest.mark.parametrize('name', NAMES)
def test_trace_grazing_faces_ragged(dsdf, name):
    """dsdf.trace (differentiable) against c_oracle.trace (fp64) for rays grazing the +x / +y faces: hit flags, its_t and the warp
    outputs; gates 2 x the fp32 C build's own error (hit flags: 2 x its mismatches, at least 2)."""
    case = ragged_case(name)
    g32 = case['grid'].float().numpy()
    o, d, m = _grazing_rays(g32.shape, RAGGED[name][-1] + 1)
    ref = c_oracle.trace(P.clib(True), g32, o, d, m)
    c32 = c_oracle.trace(P.clib(False), g32, o, d, m)
    out = {k: v.cpu().numpy() for k, v in dsdf.trace(_grid(dsdf, case), torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(),
                                                      torch.from_numpy(m).cuda(), True).items()}
    fin = np.isfinite(ref['its_t'])
    assert fin.sum() > 500 and (~fin).sum() > 500                       # the rays do graze: many hit, many miss
    flips, flips32 = int((np.isfinite(out['its_t']) != fin).sum()), int((np.isfinite(c32['its_t']) != fin).sum())
    assert flips <= max(2, 2 * flips32), (flips, flips32)
    assert (out['steps'] != ref['steps']).mean() <= max(2 * (c32['steps'] != ref['steps']).mean(), 0.01)      # (test_trace_gpu: 0.99)
    both = fin & np.isfinite(out['its_t']) & np.isfinite(c32['its_t'])
    wf = np.isfinite(ref['warp_t']) & np.isfinite(out['warp_t']) & np.isfinite(c32['warp_t'])
    bad = []
    for k in ('its_t', 'warp_t', 'warp_weight', 'warp_t_d', 'warp_weight_d'):
        msk = both if k == 'its_t' else wf
        e, f = P.rel_l2(out[k][msk], ref[k][msk]), P.rel_l2(c32[k][msk], ref[k][msk])
        P.record('trace_ragged', case=name, output=k, err=e, floor=f, rays=int(msk.sum()))
        if not e <= max(2 * f, 1e-6):
            bad.append((k, e, f))
    assert not bad, bad


# ------------------------------------------------------------------ primal (persistent workers, cell cache, proofs, hand-off)
@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('integ', [O.SILHOUETTE, O.SIMPLE_SHADING])
@pytest.mark.parametrize('spp', [64, 256])
def test_primal_ragged(dsdf, name, integ, spp):
    """All views of a case in one call, proofs on and off, each view against the fp64 oracle; hit counts against the oracle's;
    proof-on lanes marched inside the box <= the oracle's; proof on == proof off."""
    case = ragged_case(name, spp)
    grid, sens = _grid(dsdf, case), _sensors(dsdf, case)
    offs = case['offsets_all'].cuda()
    son, soff = dsdf.new_stats('cuda'), dsdf.new_stats('cuda')
    a = dsdf.render_forward(grid, sens, spp, offsets=offs, integrator=integ, stats=son).cpu().numpy()
    b = dsdf.render_forward(grid, sens, spp, offsets=offs, integrator=integ, stats=soff, empty_space_skip=False).cpu().numpy()
    don, doff = dsdf.stats_dict(son), dsdf.stats_dict(soff)
    hits = lanes = bbox = 0
    errs = []
    for k, v in enumerate(case['views']):
        ref, st = P.c_forward(v, integ, True)
        hits, lanes, bbox = hits + st['hits'], lanes + st['lanes'], bbox + st['bbox']
        # (films of ~1000 pixels: ONE eps-grazing sample that flips against fp64 -- the hit counts below allow two -- is ~1e-4 of the
        # image at spp 256; at most two flip-shaped windows are set aside, tests/precision.py image_rel_l2_but_flips)
        e_on, r_on, w_on = P.image_rel_l2_but_flips(a[k], ref, FWD_TOL, spp)
        e_off, r_off, w_off = P.image_rel_l2_but_flips(b[k], ref, FWD_TOL, spp)
        P.record('image_ragged', case=v['name'], integ=integ, spp=spp, err=e_on, err_rest=r_on, windows=w_on, err_no_skip=e_off,
                 err_rest_no_skip=r_off, windows_no_skip=w_off)
        errs.append((v['name'], r_on, r_off, e_on, e_off))
    P.record('hits_ragged', case=case['name'], integ=integ, spp=spp, hits_hip=don['hits'], hits_no_skip=doff['hits'], hits_oracle=hits,
             bbox_lanes_hip=don['bbox_lanes'], bbox_oracle=bbox, tail_rays=don['tail_rays'], tail_rays_no_skip=doff['tail_rays'])
    assert all(r_on < FWD_TOL and r_off < FWD_TOL for _, r_on, r_off, _, _ in errs), errs
    assert doff['lanes'] == lanes
    assert abs(doff['hits'] - hits) <= max(2, 2e-6 * lanes), (doff['hits'], hits)
    assert abs(don['hits'] - hits) <= max(2, 2e-6 * lanes), (don['hits'], hits)
    assert don['bbox_lanes'] <= bbox, (don['bbox_lanes'], bbox)
    assert P.rel_l2(a, b) < 1e-6


def test_tail_hand_off_runs_on_ragged_grids(dsdf):
    """The hand-off of the last long rays to the tail kernels is part of what the ragged primal tests cover: it runs on them."""
    tails = {}
    for name in NAMES:
        case = ragged_case(name)
        st = dsdf.new_stats('cuda')
        dsdf.render_forward(_grid(dsdf, case), _sensors(dsdf, case), case['spp'], offsets=case['offsets_all'].cuda(), stats=st)
        tails[name] = dsdf.stats_dict(st)['tail_rays']
    P.record('tail_rays_ragged', **tails)
    assert max(tails.values()) > 0, tails


# films fine enough for the hit proof on the ragged grids (tests/test_proof_host.py RAGGED_FILMS)
@pytest.mark.parametrize('name,W,H', [('rag_x1', 240, 234), ('rag_x2', 252, 246)])
def test_proofs_exact_on_ragged_grids_fine_film(dsdf, name, W, H):
    """Films for which the 4^3 minima AND the hit proof are on: the partial last blocks of both bounds decide pixels of the +x / +y
    faces.  All proofs vs the empty-space proof alone vs none: the same hits and images; the proofs do remove work."""
    case = ragged_case(name)
    grid = _grid(dsdf, case)
    sens = dsdf.get_regular_cameras(case['ncam'], resx=W, resy=H)[:2]
    seeds = [5, 6]
    st = {m: dsdf.new_stats('cuda') for m in ('all', 'empty', 'none')}
    a = dsdf.render_forward(grid, sens, 64, seeds=seeds, stats=st['all']).cpu().numpy()
    b = dsdf.render_forward(grid, sens, 64, seeds=seeds, stats=st['empty'], empty_space_skip='empty-only').cpu().numpy()
    c = dsdf.render_forward(grid, sens, 64, seeds=seeds, stats=st['none'], empty_space_skip=False).cpu().numpy()
    d = {m: dsdf.stats_dict(v) for m, v in st.items()}
    P.record('proofs_ragged', case=name, W=W, H=H, **{f'{m}_{k}': d[m][k] for m in d for k in ('hits', 'lanes', 'all_steps')})
    assert d['all']['hits'] == d['empty']['hits'] == d['none']['hits'] > 0
    assert P.rel_l2(a, c) < 1e-6 and P.rel_l2(b, c) < 1e-6
    assert d['all']['lanes'] < d['empty']['lanes'] < d['none']['lanes']        # both proofs take pixels off the work list


# ------------------------------------------------------------------ gradient pass
SWEEP_TAILS = {}                # (case, integrator, reparam) -> rays the gradient sweep handed to the tail kernel
@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('integ,reparam', [(O.SILHOUETTE, True), (O.SILHOUETTE, False), (O.SIMPLE_SHADING, True)])
def test_gradient_pass_ragged(dsdf, name, integ, reparam):
    """dL/dsdf of each view against the fp64 oracle with the plain gate of the oracle-sized cases (P.check_gradient: 2 x the measured
    fp32 floor, never below 1e-4) and the gradient pass's own image (at most two single-sample flips set aside, tests/precision.py
    image_rel_l2_but_flips).  The grids are the ragged ones with the surface 0.6 voxel short of the +x / +y faces (cases.ragged_grid,
    walls=False): it still runs through the last cell of every axis -- the last x chunk, the partial blocks -- but never meets a wall.
    Where it does (the primal tests above), the grazing samples along the crease carry 1/denom^3 weights that make ANY fp32 gradient a
    heavy-tailed draw: the fp32 C build itself is 0.2 off the fp64 one on rag_x3 view 0 ("Surface on a box
    wall").  A view that still misses the plain gate passes only if the excess is attributed to named ill-conditioned samples
    (_attributed_to_ill_conditioned_samples)."""
    case = ragged_case(name, walls=False)
    grid = _grid(dsdf, case)
    fails = []
    tails = 0
    for v, sen in zip(case['views'], _sensors(dsdf, case)):
        st = dsdf.new_stats('cuda')
        gg, img = dsdf.render_backward(grid, sen, v['spp'], v['grad_image'].cuda()[None], offsets=v['offsets'].cuda(), integrator=integ,
                                       reparam=reparam, return_image=True, stats=st)
        tails += dsdf.stats_dict(st)['tail_rays']
        gg = gg.cpu().numpy()
        r = P.reference_gradient(v, integ, reparam)
        e_plain, e_rest, windows = P.image_rel_l2_but_flips(img[0].cpu().numpy(), r['img64'], FWD_TOL, v['spp'])
        P.record('image_grad_pass_ragged', case=v['name'], integ=integ, reparam=reparam, err=e_plain, err_rest=e_rest,
                 flips=len(windows), windows=windows)
        if not e_rest < FWD_TOL:
            fails.append(('image', v['name'], e_plain, e_rest, windows))
        assert np.isfinite(gg).all()
        if integ == O.SILHOUETTE and not reparam:
            if np.abs(gg).max() != 0:                          # no reparameterisation: the silhouette has no gradient
                fails.append(('nonzero gradient', v['name']))
            continue
        ok, msg = P.check_gradient('ragged', v, integ, reparam, gg)
        if not ok:
            named, why = _attributed_to_ill_conditioned_samples(dsdf, v, grid, gg, r)
            if not named:
                fails.append((msg, why))
    assert not fails, fails
    # the sweep's hand-off to k_tail_trace_diff (whose finished samples splat their value on their own) is part of what these cases
    # cover: once every case has run, at least one has handed rays off
    SWEEP_TAILS[(name, integ, reparam)] = tails
    P.record('tail_rays_sweep_ragged', case=name, integ=integ, reparam=reparam, tail_rays=tails)
    if len(SWEEP_TAILS) == 3 * len(NAMES):
        assert max(SWEEP_TAILS.values()) > 0, SWEEP_TAILS


# a view whose plain gradient error exceeds the gate may set aside cubes only up to this share of the grid's voxels (a 7^3 cube is
# 13 % of rag_thin: one cube at most there)
MAX_SET_ASIDE = 0.15


def _attributed_to_ill_conditioned_samples(dsdf, v, grid, gg, r):
    """Both steps of tests/test_gpu_attribution.py for ONE view whose plain rel-L2 misses its gate: (1) at most K = max(3, 1e-5 x
    lanes) cubes of 7^3 voxels around the largest errors, no more than MAX_SET_ASIDE of the voxels, set aside leave a rest within
    2 x the fp32 C build's error with the same budget; (2) every cube set aside holds a sample whose STANDALONE per-ray trace (dsdf_trace)
    disagrees with the fp64 oracle on identical fp32 rays by more than 30 x the bulk median -- an ill-conditioned sample.  A lookup or
    gradient-kernel bug in the last x chunk or a partial block leaves either a rest above the gate or a cube no such sample explains.
    Returns (True, record) or (False, reason)."""
    from test_gpu_attribution import _per_ray_disagreement
    lanes = int(v['offsets'].shape[0])
    K = max(3, int(np.ceil(1e-5 * lanes)))
    floor_k, _, _ = P.greedy_blocks(r['g32'], r['g64'], 0.0, K)
    gate = max(P.FLOOR_FACTOR * floor_k, P.NORTH_STAR)
    rest, centres, keep = P.greedy_blocks(gg, r['g64'], gate, K)
    frac = float(1.0 - keep.mean())
    info = dict(case=v['name'], K=K, removed=len(centres), centres=centres, err_rest=rest, floor_rest=floor_k, gate=gate,
                removed_voxel_fraction=frac)
    if not (rest <= gate and frac <= MAX_SET_ASIDE):
        P.record('grad_attributed_ragged', named=False, **info)
        return False, info
    rays = P.lane_rays(v)
    o, d, maxt = rays
    tr = dsdf.trace(grid, o.cuda(), d.cuda(), maxt.cuda(), differentiable=True)
    wt = tr['warp_t'].cpu()
    idx = (torch.isfinite(wt) & (tr['warp_weight'].cpu() > 0)).nonzero()[:, 0]
    x = o[idx] + wt[idx, None] * d[idx]
    rz, ry, rx = v['grid'].shape
    cell = torch.floor(x * torch.tensor([rx, ry, rz], dtype=torch.float32) - 0.5).long()
    bulk_l = idx[torch.randperm(len(idx), generator=torch.Generator().manual_seed(0))[:20000]].numpy()
    bulk, _, _ = _per_ray_disagreement(dsdf, v, grid, rays, bulk_l)
    med = float(np.median(bulk[bulk > 0])) if (bulk > 0).any() else 0.0
    worst = []
    for (cz, cy, cx) in centres:
        m = ((cell[:, 0] - cx).abs() <= 4) & ((cell[:, 1] - cy).abs() <= 4) & ((cell[:, 2] - cz).abs() <= 4)
        cand = idx[m].numpy()
        dis = _per_ray_disagreement(dsdf, v, grid, rays, cand)[0] if len(cand) else np.zeros(1)
        worst.append(float(dis.max()))
    info.update(bulk_median=med, disagreement=worst)
    named = all(w > 30.0 * med for w in worst)
    P.record('grad_attributed_ragged', named=named, **info)
    return named, info


# ------------------------------------------------------------------ sdf_direct_reparam (wavefront, fused MIS worker)
DIRECT_CASE = 'rag_x1'          # rx != rz: the cell table's x size differs from its z size
ALBEDO_SHAPE = (7, 5, 9)


def _direct_inputs(case, seed=17):
    views = case['views'][:2]
    gen = torch.Generator().manual_seed(seed)
    albedo = torch.rand(*ALBEDO_SHAPE, 3, generator=gen, dtype=torch.float32) * 0.6 + 0.2
    emit = [torch.rand(v['offsets'].shape[0], 2, generator=gen, dtype=torch.float32) for v in views]
    bsdf = [torch.rand(v['offsets'].shape[0], 2, generator=gen, dtype=torch.float32) for v in views]
    return views, dict(albedo=albedo, emitter_u=emit, bsdf_u=bsdf, env=(1.0, 0.9, 0.8))


def _c_direct(lib, v, k, ex, hide, grads, mis=False):
    a = (v['grid'].float().numpy(), v['cam'].params(), v['W'], v['H'], v['spp'], v['offsets'].numpy(), ex['emitter_u'][k].numpy(),
         ex['albedo'].numpy())
    if not grads:
        return c_oracle.render_direct(lib, *a, env=ex['env'], hide_emitters=hide, bsdf_u=ex['bsdf_u'][k].numpy() if mis else None)
    return c_oracle.render_direct_backward(lib, *a, v['grad_image'].numpy(), env=ex['env'], hide_emitters=hide)


@pytest.mark.parametrize('hide', [False, True])
def test_direct_wavefront_ragged(dsdf, hide):
    """Two views of a ragged grid with a ragged albedo volume in one call of the wavefront sdf_direct_reparam (spp 64; hide_emitters
    False also fills the film's missed samples with the environment, k_film_env, with the proofs on): primal image, gradient-pass
    image, dL/dsdf and dL/dalbedo (summed over the views) against the fp64 C oracle; gradient gates 2 x (fp32 build vs fp64)."""
    case = ragged_case(DIRECT_CASE)
    views, ex = _direct_inputs(case)
    grid, sens = _grid(dsdf, case), _sensors(dsdf, case, views)
    sh = dsdf.Shading(ex['albedo'].cuda(), ex['env'], hide_emitters=hide)
    offs = torch.cat([v['offsets'] for v in views]).cuda()
    emit = torch.cat(ex['emitter_u']).cuda()
    gi = torch.stack([v['grad_image'] for v in views]).cuda()
    img = dsdf.render_forward(grid, sens, 64, offsets=offs, integrator='sdf_direct_reparam', shading=sh, emitter_samples=emit).cpu().numpy()
    galb = torch.zeros_like(sh.albedo)
    gg, gimg = dsdf.render_backward(grid, sens, 64, gi, offsets=offs, integrator='sdf_direct_reparam', return_image=True, shading=sh,
                                    emitter_samples=emit, grad_albedo=galb)
    gg, gimg, galb = gg.cpu().numpy(), gimg.cpu().numpy(), galb.cpu().numpy()
    gd = {True: 0.0, False: 0.0}
    ga = {True: 0.0, False: 0.0}
    errs = []
    for k, v in enumerate(views):
        ref = _c_direct(P.clib(True), v, k, ex, hide, False)
        for double in (True, False):
            d_, a_, im = _c_direct(P.clib(double), v, k, ex, hide, True)
            gd[double] = gd[double] + d_
            ga[double] = ga[double] + a_
            if double:
                img64 = im
        errs.append((v['name'], P.rel_l2(img[k], ref), P.rel_l2(gimg[k], img64)))
    ed, ea = P.rel_l2(gg, gd[True]), P.rel_l2(galb, ga[True])
    fd, fa = P.rel_l2(gd[False], gd[True]), P.rel_l2(ga[False], ga[True])
    tol_d, tol_a = max(P.FLOOR_FACTOR * fd, P.NORTH_STAR), max(P.FLOOR_FACTOR * fa, P.NORTH_STAR)
    P.record('direct_ragged', case=DIRECT_CASE, hide=hide, images=errs, err_data=ed, floor_data=fd, tol_data=tol_d, err_albedo=ea,
             floor_albedo=fa, tol_albedo=tol_a)
    assert all(e1 < FWD_TOL and e2 < FWD_TOL for _, e1, e2 in errs), errs
    assert ed <= tol_d, (ed, tol_d)
    assert ea <= tol_a, (ea, tol_a)
    assert np.isfinite(gg).all() and np.isfinite(galb).all()


def test_direct_mis_ragged(dsdf):
    """use_mis at spp 64 (the fused worker k_render_items<..., true, ...>: emitter + BSDF sampling) on the ragged grid, two views."""
    case = ragged_case(DIRECT_CASE)
    views, ex = _direct_inputs(case)
    grid, sens = _grid(dsdf, case), _sensors(dsdf, case, views)
    sh = dsdf.Shading(ex['albedo'].cuda(), ex['env'], use_mis=True)
    img = dsdf.render_forward(grid, sens, 64, offsets=torch.cat([v['offsets'] for v in views]).cuda(), integrator='sdf_direct_reparam',
                              shading=sh, emitter_samples=torch.cat(ex['emitter_u']).cuda(),
                              bsdf_samples=torch.cat(ex['bsdf_u']).cuda()).cpu().numpy()
    errs = [(v['name'], P.rel_l2(img[k], _c_direct(P.clib(True), v, k, ex, False, False, mis=True))) for k, v in enumerate(views)]
    P.record('direct_mis_ragged', case=DIRECT_CASE, images=errs)
    assert all(e < FWD_TOL for _, e in errs), errs


CHILD = r'''
import os, sys, numpy as np, torch
root = sys.argv[1]
for p in (os.path.join(root, 'differentiable-sdf-rendering_amd', 'python'), os.path.join(root, 'oracle'), os.path.join(root, 'tests')):
    sys.path.insert(0, p)
import dsdf
import test_gpu_ragged as T
from cases import ragged_case
case = ragged_case(T.DIRECT_CASE)
views, ex = T._direct_inputs(case)
cams = dsdf.get_regular_cameras(case['ncam'], resx=case['W'], resy=case['H'])
sens = [cams[v['icam']] for v in views]
grid = dsdf.SdfGrid(case['grid'].float().cuda())
sh = dsdf.Shading(ex['albedo'].cuda(), ex['env'])
st = dsdf.new_stats('cuda')
img = dsdf.render_forward(grid, sens, 64, offsets=torch.cat([v['offsets'] for v in views]).cuda(), integrator='sdf_direct_reparam',
                          shading=sh, emitter_samples=torch.cat(ex['emitter_u']).cuda(), stats=st)
sd = dsdf.stats_dict(st)
torch.cuda.synchronize()
np.savez(sys.argv[2], img=img.cpu().numpy(), counts=np.array([sd['lanes'], sd['tail_steps'], sd['tail_rays']], dtype=np.int64))
'''


def test_direct_shadow_stream_without_cell_table(dsdf, tmp_path):
    """k_shadow_stream<false> (no cell table: grids above ~406^3, a workspace halved on OOM, DSDF_CELL_TABLE=0) and <true>, each in a
    fresh process on the same inputs: both images against the fp64 oracle, and against each other to the film atomics' order; the
    same shadow rays and steps."""
    script = tmp_path / 'child.py'
    script.write_text(CHILD)
    for tag, table in (('table', None), ('no_table', '0')):
        env = {k: v for k, v in os.environ.items() if k != 'DSDF_CELL_TABLE'}
        if table is not None:
            env['DSDF_CELL_TABLE'] = table
        r = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / f'{tag}.npz')], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
    a, b = np.load(tmp_path / 'table.npz'), np.load(tmp_path / 'no_table.npz')
    case = ragged_case(DIRECT_CASE)
    views, ex = _direct_inputs(case)
    errs = []
    for k, v in enumerate(views):
        ref = _c_direct(P.clib(True), v, k, ex, False, False)
        errs.append((v['name'], P.rel_l2(a['img'][k], ref), P.rel_l2(b['img'][k], ref)))
    P.record('direct_no_cell_table_ragged', case=DIRECT_CASE, images=errs, counts_table=a['counts'].tolist(), counts_no_table=b['counts'].tolist())
    assert all(e1 < FWD_TOL and e2 < FWD_TOL for _, e1, e2 in errs), errs
    assert (a['counts'] == b['counts']).all() and a['counts'][2] > 1000, (a['counts'], b['counts'])
    assert P.rel_l2(b['img'], a['img']) < 2e-6
