"""GPU parity: the HIP path (through the C-ABI / ctypes shim) against the oracle on
identical seeded inputs, plus size-independent properties at larger sizes.
Tolerances: forward 1e-4 relative L2 (north_star); gradients max(2 x measured fp32 floor, 1e-4)
per case against the fp64 oracle (tests/precision.py; config sizes: test_gpu_config_size.py)."""
import numpy as np
import pytest
import torch

import sdf_oracle as O
from cases import make_case, oracle_backward, oracle_forward
import precision as P
from conftest import rel_l2

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    assert torch.cuda.is_available()
    return m


def dev_grid(dsdf, case):
    return dsdf.SdfGrid(case['grid'].float().cuda())


def sensor(dsdf, case):
    return dsdf.get_regular_cameras(case['ncam'], resx=case['W'], resy=case['H'])[case['icam']]


def test_eval_cubic_gpu(dsdf):
    grid = O.blob_grid(24, n=5, seed=4)
    pts = (torch.rand(20000, 3, dtype=torch.float64) * 1.1 - 0.05).float()
    g = dsdf.SdfGrid(grid.float().cuda())
    v, gr, H = dsdf.eval_cubic(g, pts.cuda(), 2)
    vo, go, Ho = O.eval_cubic(grid, pts.double(), 2)
    Ho6 = torch.stack([Ho[:, 0, 0], Ho[:, 1, 1], Ho[:, 2, 2], Ho[:, 0, 1], Ho[:, 0, 2], Ho[:, 1, 2]], -1)
    assert rel_l2(v.cpu(), vo) < 1e-6 and rel_l2(gr.cpu(), go) < 1e-5 and rel_l2(H.cpu(), Ho6) < 1e-5
    v0, _, _ = dsdf.eval_cubic(g, pts.cuda(), 0)
    assert rel_l2(v0.cpu(), vo) < 1e-6


def test_trace_gpu(dsdf):
    """A2 per ray: every output of SDFBase.ray_intersect -- including the 22-accumulator derivative state behind
    warp_t_d / warp_weight_d -- against the fp64 oracle; gates = max(2 x the fp32 C restatement's own error, 1e-6)."""
    import c_oracle
    case = make_case('blob32')
    o32, d32, m32, ref = P.silhouette_rays(case, n=8000, seed=11)
    c32 = c_oracle.trace(P.clib(False), case['grid'].float().numpy(), o32.numpy(), d32.numpy(), m32.numpy())
    out = dsdf.trace(dev_grid(dsdf, case), o32.cuda(), d32.cuda(), m32.cuda(), True)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    fin = torch.isfinite(ref['its_t']).numpy()
    assert np.array_equal(np.isfinite(out['its_t']), fin)
    assert (out['steps'] == ref['steps'].numpy()).mean() > 0.99
    wf = torch.isfinite(ref['warp_t']).numpy()
    assert (np.isfinite(out['warp_t']) == wf).mean() > 0.999
    both = wf & np.isfinite(out['warp_t']) & np.isfinite(c32['warp_t'])
    assert both.sum() > 1000
    for k in ('its_t', 'warp_t', 'warp_weight', 'warp_t_d', 'warp_weight_d'):
        m = fin if k == 'its_t' else both
        b = ref[k].numpy()[m]
        e, f = rel_l2(out[k][m], b), rel_l2(c32[k][m], b)
        P.record('trace', case='blob32', output=k, err=e, floor=f)
        assert e <= max(2 * f, 1e-6), (k, e, f)
    plain = dsdf.trace(dev_grid(dsdf, case), o32.cuda(), d32.cuda(), m32.cuda(), False)['its_t'].cpu().numpy()
    assert np.array_equal(np.isfinite(plain), fin) and rel_l2(plain[fin], out['its_t'][fin]) < 1e-6


def test_warp_eval_gpu(dsdf):
    """A9 per ray through the C-ABI (dsdf_warp_eval): (i) on the oracle's trace outputs, isolating WarpField2D.eval;
    (ii) on the HIP path's own dsdf_trace outputs (per-ray end to end)."""
    case = make_case('blob32')
    o32, d32, m32, tr = P.silhouette_rays(case, n=8000, seed=12)
    tr32 = {k: v.float() for k, v in tr.items() if k != 'steps'}
    grid = dev_grid(dsdf, case)
    out = dsdf.warp_eval(grid, o32.cuda(), d32.cuda(), {k: v.cuda() for k, v in tr32.items()})
    P.check_warp_coefficients('hip', case, o32, d32, tr32, {k: v.cpu().numpy() for k, v in out.items()})
    own = dsdf.trace(grid, o32.cuda(), d32.cuda(), m32.cuda(), True)
    out2 = dsdf.warp_eval(grid, o32.cuda(), d32.cuda(), own)
    a1, a2 = out['active'].cpu().numpy() != 0, out2['active'].cpu().numpy() != 0
    assert (a1 != a2).mean() < 2e-3
    m = a1 & a2
    for k in ('cdir', 'a', 'b', 'div'):
        assert rel_l2(out2[k].cpu().numpy()[m], out[k].cpu().numpy()[m]) < 5e-3, k     # fp32 trace outputs vs fp64 ones as inputs


def test_surface_interaction_gpu(dsdf):
    """A6 per ray through the C-ABI (dsdf_surface_interaction) against SDFBase.compute_surface_interaction of the oracle:
    p, n, and dt/dv = 1 / (g . -d) by autograd."""
    case = make_case('blob32')
    o32, d32, m32, tr = P.silhouette_rays(case, n=4000, seed=13)
    t32 = tr['its_t'].float()
    hit = torch.isfinite(t32)
    out = dsdf.surface_interaction(dev_grid(dsdf, case), o32.cuda(), d32.cuda(), t32.cuda())
    out = {k: v.cpu().numpy() for k, v in out.items()}
    data = case['grid'].float().double().clone().requires_grad_(True)
    oh, dh, th = o32.double()[hit], d32.double()[hit], t32.double()[hit]
    t_att, p, n = O.compute_surface_interaction(O.Grid3d(data), oh, dh, th, torch.ones_like(th, dtype=torch.bool))
    h = hit.numpy()
    assert rel_l2(out['p'][h], p.detach().numpy()) < 1e-6 and rel_l2(out['n'][h], n.detach().numpy()) < 1e-5
    assert np.abs(out['p'][~h]).max(initial=0.0) == 0.0 and np.abs(out['t_coef'][~h]).max(initial=0.0) == 0.0
    # dt/dv: t = replace_grad(t, v(p)/detach(g.-d)) -> sum_k t_k back-propagates t_coef_k * W_taps(p_k) into the grid
    t_att.sum().backward()
    gsum = data.grad
    v, g, _ = dsdf.eval_cubic(dev_grid(dsdf, case), torch.tensor(out['p'][h]).cuda(), 1)
    assert rel_l2(out['grad'][h], g.cpu().numpy()) < 1e-6
    tc = 1.0 / (-(g.cpu().double() * dh).sum(-1))
    assert rel_l2(out['t_coef'][h], tc.numpy()) < 1e-5
    # scatter the HIP coefficients with the oracle's weights: same grid gradient as autograd
    data2 = case['grid'].float().double().clone().requires_grad_(True)
    vv, _ = O.Grid3d(data2).eval_and_grad(torch.tensor(out['p'][h], dtype=torch.float64))
    (vv * torch.tensor(out['t_coef'][h], dtype=torch.float64)).sum().backward()
    assert rel_l2(data2.grad.numpy(), gsum.numpy()) < 1e-4


@pytest.mark.parametrize('name', ['sphere16', 'blob32', 'blob32_spp64', 'blob48_rect', 'blob32_spp192', 'blob32_spp2'])
@pytest.mark.parametrize('integ', [O.SILHOUETTE, O.SIMPLE_SHADING])
def test_render_forward_gpu(dsdf, name, integ):
    case = make_case(name)
    ref, aux = oracle_forward(case, integ)
    img = dsdf.render_forward(dev_grid(dsdf, case), sensor(dsdf, case), case['spp'], offsets=case['offsets'].cuda(),
                              integrator=integ)[0]
    assert rel_l2(img.cpu(), ref) < FWD_TOL
    # step statistics are compared with the empty-space proof off (it skips provably missing rays)
    stats = dsdf.new_stats('cuda')
    img2 = dsdf.render_forward(dev_grid(dsdf, case), sensor(dsdf, case), case['spp'], offsets=case['offsets'].cuda(),
                               integrator=integ, stats=stats, empty_space_skip=False)[0]
    assert rel_l2(img2.cpu(), ref) < FWD_TOL
    st = dsdf.stats_dict(stats)
    assert st['lanes'] == aux['lanes'] and st['hits'] == aux['hits']
    assert abs(st['all_steps'] - aux['steps']) <= 0.01 * aux['steps']      # (render kernel + tail kernels)


@pytest.mark.parametrize('name', ['sphere16', 'blob32', 'blob32_spp64', 'blob48_rect', 'blob32_spp192', 'blob32_spp2'])
@pytest.mark.parametrize('integ', [O.SILHOUETTE, O.SIMPLE_SHADING])
@pytest.mark.parametrize('reparam', [True, False])
def test_render_backward_gpu(dsdf, name, integ, reparam):
    case = make_case(name)
    gref = oracle_backward(case, integ, reparam).numpy()
    gg, img = dsdf.render_backward(dev_grid(dsdf, case), sensor(dsdf, case), case['spp'], case['grad_image'].cuda()[None],
                                   offsets=case['offsets'].cuda(), integrator=integ, reparam=reparam, return_image=True)
    ref_img, _ = oracle_forward(case, integ)
    assert rel_l2(img[0].cpu(), ref_img) < FWD_TOL         # gradient-pass image == primal image on the same samples (F8)
    gg = gg.cpu().numpy()
    if not reparam and integ == O.SILHOUETTE:
        assert np.abs(gg).max() == 0
        return
    assert np.isfinite(gg).all()
    ok, msg = P.check_gradient('hip', case, integ, reparam, gg)
    assert ok, msg
    assert rel_l2(gref, P.reference_gradient(case, integ, reparam)['g64']) < 1e-6     # both fp64 oracles agree


def test_odd_film_tail_waves_do_not_splat(dsdf):
    """Film 33x33 at spp 64: (W+4)(H+4) = 1369 pixel-waves, not a multiple of the 4 waves of a block -- the three tail
    waves past the last sample are clamped to it for the cross-lane code and must not splat.  Proof off, so
    that nothing else hides them; compared with the oracle, last pixel included."""
    W = H = 33
    gen = torch.Generator().manual_seed(9)
    offs = torch.rand((W + 4) * (H + 4) * 64, 2, generator=gen)
    grid64 = O.blob_grid(32, n=6, seed=1)
    origin = O.regular_camera_origins(3)[1]
    cam = O.Camera(origin).rounded()
    import c_oracle
    ref, _ = c_oracle.render(P.clib(True), grid64.float().numpy(), cam.params(), W, H, 64, offs.numpy(), O.SIMPLE_SHADING)
    sen = dsdf.Sensor(origin, resx=W, resy=H)
    for skip in (False, True):
        img = dsdf.render_forward(dsdf.SdfGrid(grid64.float().cuda()), sen, 64, offsets=offs.cuda(), integrator=O.SIMPLE_SHADING,
                                  empty_space_skip=skip)[0].cpu().numpy()
        assert rel_l2(img, ref) < FWD_TOL
        assert np.abs(img[-2:, -2:] - ref[-2:, -2:]).max() < 1e-5


@pytest.mark.parametrize('spp', [64, 4])
def test_tile_split_equals_whole_view_gpu(dsdf, spp):
    """Multi-GPU pixel-tile split (dsdf_render_film / dsdf_develop / dsdf_grad_sweep / dsdf_grad_backward): two row windows of
    the film block, rendered one after the other like two ranks would, add up to the un-split render -- image and dL/dsdf --
    on the persistent-worker path (spp 64) and on the general path (spp 4)."""
    case = make_case('blob48_rect')
    W, H = case['W'], case['H']
    grid = dev_grid(dsdf, case)
    sens = dsdf.get_regular_cameras(12, resx=W, resy=H)[4:6]
    seeds = [21, 22]
    for integ in (O.SILHOUETTE, O.SIMPLE_SHADING):
        whole = dsdf.render_forward(grid, sens, spp, seeds=seeds, integrator=integ)
        gi = torch.randn(2, H, W, 3, device='cuda')
        g_whole = dsdf.render_backward(grid, sens, spp, gi, seeds=seeds, integrator=integ)
        wins = [(0, 9), (9, H + 4)]
        film = dsdf.new_film(2, W, H, integ, 'cuda')
        for rows in wins:
            dsdf.render_film(grid, sens, spp, film, rows, seeds=seeds, integrator=integ)
        img = dsdf.develop(film, W, H, integ)
        assert rel_l2(img.cpu(), whole.cpu()) < 1e-6
        film_g = dsdf.new_film(2, W, H, integ, 'cuda')
        sweeps = [dsdf.GradSweep(grid, sens, spp, rows, seeds=seeds, integrator=integ) for rows in wins]
        for sw in sweeps:
            sw.sweep(film_g)
        g = torch.zeros_like(g_whole)
        for sw in sweeps:
            sw.backward(film_g, gi, g)
        assert rel_l2(g.cpu(), g_whole.cpu()) < 1e-5
    with pytest.raises(dsdf.DsdfError):
        dsdf.render_film(grid, sens, spp, film, (5, 5), seeds=seeds)               # empty window


def test_backward_accumulates(dsdf):
    case = make_case('blob32')
    grid, sen = dev_grid(dsdf, case), sensor(dsdf, case)
    kw = dict(offsets=case['offsets'].cuda(), integrator=O.SILHOUETTE)
    g1 = dsdf.render_backward(grid, sen, case['spp'], case['grad_image'].cuda()[None], **kw)
    g2 = dsdf.render_backward(grid, sen, case['spp'], case['grad_image'].cuda()[None], grad_grid=g1.clone(), **kw)
    assert rel_l2(g2.cpu(), 2 * g1.cpu()) < 1e-5
    # linearity in grad_image (size-independent property)
    g3 = dsdf.render_backward(grid, sen, case['spp'], -3.0 * case['grad_image'].cuda()[None], **kw)
    assert rel_l2(g3.cpu(), -3.0 * g1.cpu()) < 1e-5


def test_builtin_sampler_matches_explicit_offsets(dsdf):
    """In-kernel `independent` sampler (PCG32 + sample_tea_32) == oracle's numpy restatement."""
    case = make_case('blob32')
    n = (case['W'] + 4) * (case['H'] + 4) * case['spp']
    offs = torch.tensor(O.independent_sampler_2d(77, n))
    grid, sen = dev_grid(dsdf, case), sensor(dsdf, case)
    a = dsdf.render_forward(grid, sen, case['spp'], seeds=[77], integrator=O.SIMPLE_SHADING)
    b = dsdf.render_forward(grid, sen, case['spp'], offsets=offs.cuda(), integrator=O.SIMPLE_SHADING)
    assert rel_l2(a.cpu(), b.cpu()) < 1e-6


def test_multi_view_batch_equals_single_views(dsdf):
    case = make_case('blob48_rect')
    sens = dsdf.get_regular_cameras(12, resx=case['W'], resy=case['H'])[:3]
    grid = dev_grid(dsdf, case)
    batch = dsdf.render_forward(grid, sens, 4, seeds=[5, 6, 7])
    for i, s in enumerate(sens):
        one = dsdf.render_forward(grid, s, 4, seeds=[5 + i])
        assert rel_l2(batch[i].cpu(), one[0].cpu()) < 1e-6
    gi = torch.randn(3, case['H'], case['W'], 3).cuda()
    gb = dsdf.render_backward(grid, sens, 4, gi, seeds=[9, 10, 11])
    gs = sum(dsdf.render_backward(grid, s, 4, gi[i:i + 1].contiguous(), seeds=[9 + i]) for i, s in enumerate(sens))
    assert rel_l2(gb.cpu(), gs.cpu()) < 1e-5


def test_autograd_render_op(dsdf):
    """`mi.render` semantics: primal from (seed, spp), gradient from (seed_grad, spp_grad)."""
    case = make_case('blob32')
    data = case['grid'].float().cuda().requires_grad_(True)
    grid = dsdf.SdfGrid(data)
    sen = sensor(dsdf, case)
    img = dsdf.render(data, grid, [sen], spp=16, seed=3, spp_grad=8, seed_grad=11)
    target = torch.zeros_like(img)
    loss = (img - target).abs().mean()
    loss.backward()
    assert data.grad is not None and torch.isfinite(data.grad).all() and data.grad.abs().sum() > 0
    gi = torch.sign(img.detach()) / img.numel()
    ref = dsdf.render_backward(grid, sen, 8, gi, seeds=[11])
    assert rel_l2(data.grad.cpu(), ref.cpu()) < 1e-5


def test_primal_invariance_large(dsdf):
    """Size-independent property at a bench-like size: reparam on/off gives the same image (F8),
    wave-uniform splat (spp=64) == per-lane splat path on the same samples."""
    R, W, H = 128, 96, 96
    data = O.blob_grid(R, n=16, seed=5).float().cuda()
    grid = dsdf.SdfGrid(data)
    sen = dsdf.get_regular_cameras(12, resx=W, resy=H)[3]
    a = dsdf.render_forward(grid, sen, 64, seeds=[1], reparam=True)
    b = dsdf.render_forward(grid, sen, 64, seeds=[1], reparam=False)
    assert rel_l2(a.cpu(), b.cpu()) < 1e-6
    gi = torch.randn(1, H, W, 3).cuda()
    _, img_g = dsdf.render_backward(grid, sen, 64, gi, seeds=[1], return_image=True)
    assert rel_l2(img_g.cpu(), a.cpu()) < 1e-5
    assert 0.02 < float(a.mean()) < 0.9


def test_gradient_descends_loss(dsdf):
    """End-to-end sanity at GPU-only size: a few gradient steps on a sphere SDF towards a
    bigger sphere reduce the image loss (the optimisation the reference runs)."""
    R, W, H = 64, 64, 64
    target_grid = dsdf.SdfGrid(O.sphere_grid(R, radius=0.36).float().cuda())
    data = O.sphere_grid(R, radius=0.3).float().cuda().requires_grad_(True)
    grid = dsdf.SdfGrid(data)
    sens = dsdf.get_regular_cameras(4, resx=W, resy=H)
    target = dsdf.render_forward(target_grid, sens, 64, seeds=[100, 101, 102, 103])
    losses = []
    for it in range(6):
        grid.update(data)
        img = dsdf.render(data, grid, sens, spp=64, seed=10 * it, spp_grad=16, seed_grad=10 * it + 5)
        loss = (img - target).abs().mean()
        data.grad = None
        loss.backward()
        with torch.no_grad():
            data -= 0.01 * torch.sign(data.grad)
        losses.append(float(loss))
    assert losses[-1] < 0.7 * losses[0], losses


@pytest.mark.parametrize('integ', [O.SILHOUETTE, O.SIMPLE_SHADING])
def test_gradient_vs_finite_differences_gpu(dsdf, integ):
    """The reference's own validation (figures/result_utils.py:126-161: finite differences with
    common random numbers against the reparameterised gradient), at a sample count only the GPU
    affords: directional derivative of a smooth image functional along a smooth grid perturbation
    (a translation-like bump field) -- independent of the oracle."""
    R, W, H, spp = 64, 48, 48, 2048
    base = O.sphere_grid(R, radius=0.3).float().cuda()
    lin = torch.linspace(0, 1, R, device='cuda')
    z, y, x = torch.meshgrid(lin, lin, lin, indexing='ij')
    # d(sdf)/d(theta) for a translation along +x combined with a radius change: -(x-0.5)/r + 0.5
    r = torch.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2).clamp(min=1e-3)
    direction = (-(x - 0.5) / r + 0.5).contiguous()
    sens = dsdf.get_regular_cameras(3, resx=W, resy=H)
    yy, xx = torch.meshgrid(torch.arange(H, device='cuda'), torch.arange(W, device='cuda'), indexing='ij')
    G = torch.stack([xx / W, yy / H, (xx + yy) / (W + H)], -1).float()[None].repeat(3, 1, 1, 1).contiguous()
    seeds = [11, 12, 13]
    grad = dsdf.render_backward(dsdf.SdfGrid(base), sens, spp, G, seeds=seeds, integrator=integ)
    ad = float((grad * direction).sum())

    def L(eps):
        img = dsdf.render_forward(dsdf.SdfGrid(base + eps * direction), sens, spp, seeds=seeds, integrator=integ, reparam=False)
        return float((img * G).sum())
    eps = 2e-3
    fd = (L(eps) - L(-eps)) / (2 * eps)
    assert abs(ad - fd) < 0.05 * abs(fd) + 0.5, (ad, fd)


def test_non_cubic_grid_and_rect_film(dsdf):
    """Ragged shapes: rx != ry != rz grid, W != H film, spp not a power of two."""
    torch.manual_seed(7)
    lin = [torch.linspace(0, 1, n, dtype=torch.float64) for n in (20, 28, 36)]        # (Z,Y,X)
    z, y, x = torch.meshgrid(*lin, indexing='ij')
    grid = (torch.sqrt((x - 0.5) ** 2 + (y - 0.45) ** 2 + (z - 0.55) ** 2) - 0.28).float().double()
    W, H, spp = 20, 12, 3
    offs = torch.rand((W + 4) * (H + 4) * spp, 2)
    gi = torch.randn(H, W, 3)
    origin = O.regular_camera_origins(5)[2]
    sen = dsdf.Sensor(origin, resx=W, resy=H)
    g = dsdf.SdfGrid(grid.float().cuda())
    assert g.shape == (20, 28, 36)
    for integ in (O.SILHOUETTE, O.SIMPLE_SHADING):
        cam16 = O.Camera(origin).params()
        ref = O.render(O.Grid3d(grid), O.Camera.from_params(cam16), W, H, spp, offs.double(), integ)
        img = dsdf.render_forward(g, sen, spp, offsets=offs.cuda(), integrator=integ)[0]
        assert rel_l2(img.cpu(), ref) < FWD_TOL

        def oracle(dt):
            return (O.render_backward(O.Grid3d(grid.to(dt)), O.Camera.from_params(cam16, dtype=dt), W, H, spp, offs.to(dt), gi.to(dt), integ),)
        (gref,), (tol,) = P.torch_gate(oracle)
        gg = dsdf.render_backward(g, sen, spp, gi.cuda()[None], offsets=offs.cuda(), integrator=integ)
        assert gg.shape == (20, 28, 36) and rel_l2(gg.cpu(), gref) < tol, (rel_l2(gg.cpu(), gref), tol)


def test_empty_and_degenerate_inputs(dsdf):
    g = dsdf.SdfGrid(torch.full((16, 16, 16), 0.5, device='cuda'))           # no surface anywhere
    sen = dsdf.get_regular_cameras(2, resx=16, resy=16)
    img = dsdf.render_forward(g, sen, 64, seeds=[1, 2])
    assert float(img.abs().max()) == 0.0
    gg = dsdf.render_backward(g, sen, 64, torch.ones(2, 16, 16, 3, device='cuda'), seeds=[3, 4], integrator=O.SIMPLE_SHADING)
    assert float(gg.abs().max()) == 0.0 and torch.isfinite(gg).all()
    inside = dsdf.SdfGrid(torch.full((16, 16, 16), -0.5, device='cuda'))     # solid block: every bbox ray hits at entry
    img = dsdf.render_forward(inside, sen[0], 64, seeds=[5])
    assert abs(float(img.max()) - 1.0) < 1e-5 and torch.isfinite(img).all()      # value and weight sums differ by fp32 rounding
    # zero rays / zero points are no-ops
    e = torch.empty(0, 3, device='cuda')
    out = dsdf.trace(g, e, e, torch.empty(0, device='cuda'))
    assert out['its_t'].numel() == 0
    v, gr, H = dsdf.eval_cubic(g, e, 2)
    assert v.numel() == 0 and H.shape == (0, 6)
    # a ray that misses the bounding box / points far outside the grid (clamped texture)
    o = torch.tensor([[3.0, 3.0, 3.0]], device='cuda'); d = torch.tensor([[1.0, 0.0, 0.0]], device='cuda')
    t = dsdf.trace(g, o, d, torch.full((1,), 1e4, device='cuda'))
    assert torch.isinf(t['its_t']).all() and torch.isinf(t['warp_t']).all() and float(t['warp_weight']) == 0.0
    far = dsdf.eval_cubic(g, torch.tensor([[-5.0, 7.0, 0.5]], device='cuda'), 1)
    assert abs(float(far[0]) - 0.5) < 1e-6 and float(far[1].abs().max()) == 0.0
    with pytest.raises(dsdf.DsdfError):                                       # reparam.py:48-50 wavefront limit
        dsdf.render_forward(g, dsdf.Sensor([2.5, 1, 0.5], resx=4096, resy=4096), 128, seeds=[0])
    with pytest.raises(dsdf.DsdfError):
        dsdf.render_forward(g, sen, 4, seeds=[1])                             # one seed for two views


def test_large_spp_not_multiple_of_64(dsdf):
    """Per-lane splat path (spp % 64 != 0) against the wave-uniform path on the same samples."""
    R, W, H, spp = 64, 40, 40, 96
    data = O.blob_grid(R, n=10, seed=2).float().cuda()
    g = dsdf.SdfGrid(data)
    sen = dsdf.get_regular_cameras(4, resx=W, resy=H)[1]
    n = (W + 4) * (H + 4)
    # (seeded: the comparison of two fp32 evaluations that differ in lane order is a draw of a heavy-tailed variable -- round 5 saw
    # 1.1e-4 and 5.1e-4 on unseeded offsets when the two kernels' code had drifted apart -- so the draw is fixed)
    offs = torch.rand(n * spp, 2, device='cuda', generator=torch.Generator(device='cuda').manual_seed(7))
    a = dsdf.render_forward(g, sen, spp, offsets=offs)                        # 96 spp: per-lane path
    # the same samples re-ordered as 192 spp (multiple of 64) by duplicating each sample: identical image
    offs2 = offs.reshape(n, spp, 2).repeat_interleave(2, dim=1).reshape(-1, 2).contiguous()
    b = dsdf.render_forward(g, sen, 2 * spp, offsets=offs2)                   # 192 spp: wave-uniform + cell cache
    assert rel_l2(a.cpu(), b.cpu()) < 1e-5
    gi = torch.randn(1, H, W, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(8))
    ga = dsdf.render_backward(g, sen, spp, gi, offsets=offs)
    gb = dsdf.render_backward(g, sen, 2 * spp, gi, offsets=offs2)
    assert rel_l2(ga.cpu(), gb.cpu()) < 1e-4


@pytest.mark.parametrize('integ', [O.SILHOUETTE, O.SIMPLE_SHADING])
@pytest.mark.parametrize('R,W', [(128, 128), (64, 160)])      # pixel footprint selects the 8^3 / the 4^3 min-grid
def test_empty_space_skip_is_exact(dsdf, integ, R, W):
    """The per-pixel empty-space proof (coarse dilated min-grid) must not change any result: images and
    gradients with and without it agree to atomic-ordering noise, while far fewer steps are traced."""
    H, spp = W, 64
    data = O.blob_grid(R, n=16, seed=5).float().cuda()
    grid = dsdf.SdfGrid(data)
    sens = dsdf.get_regular_cameras(6, resx=W, resy=H)[:3]
    seeds = [3, 4, 5]
    sa, sb = dsdf.new_stats('cuda'), dsdf.new_stats('cuda')
    a = dsdf.render_forward(grid, sens, spp, seeds=seeds, integrator=integ, stats=sa)
    b = dsdf.render_forward(grid, sens, spp, seeds=seeds, integrator=integ, stats=sb, empty_space_skip=False)
    assert rel_l2(a.cpu(), b.cpu()) < 1e-6
    da, db = dsdf.stats_dict(sa), dsdf.stats_dict(sb)
    # `lanes` counts the samples that are generated at all: with the proof on, pixels whose whole +-4 neighbourhood is proven
    # empty are not on the work list
    assert da['hits'] == db['hits'] and da['lanes'] < db['lanes'] and db['lanes'] == 3 * (W + 4) * (H + 4) * spp
    assert da['all_steps'] < 0.8 * db['all_steps']                     # a good part of the image is provably empty
    gi = torch.randn(3, H, W, 3, device='cuda')
    ga, ia = dsdf.render_backward(grid, sens, spp, gi, seeds=seeds, integrator=integ, return_image=True)
    gb, ib = dsdf.render_backward(grid, sens, spp, gi, seeds=seeds, integrator=integ, return_image=True, empty_space_skip=False)
    assert rel_l2(ia.cpu(), ib.cpu()) < 1e-6
    assert rel_l2(ga.cpu(), gb.cpu()) < 1e-5
    # low-resolution film on a fine grid: the pixel footprint exceeds the dilation margin -> proof disabled, same result
    lo = dsdf.get_regular_cameras(6, resx=12, resy=12)[0]
    c = dsdf.render_forward(grid, lo, spp, seeds=[1], integrator=integ)
    d = dsdf.render_forward(grid, lo, spp, seeds=[1], integrator=integ, empty_space_skip=False)
    assert rel_l2(c.cpu(), d.cpu()) < 1e-6


@pytest.mark.parametrize('spp', [4, 16, 64, 256])
def test_hit_proof_is_exact(dsdf, spp):
    """The hit proof of the silhouette primal (csrc/dsdf_proof.h: pixels whose every sample provably hits are not marched) must not
    change any result: the SAME number of hits and the same image as with the empty-space proof alone and as without any proof
    -- through the work-list kernel (spp 64 / 256) and the general pass (spp 4) -- while far fewer steps are traced.  The other
    integrators consume the hit distance and must not be affected at all."""
    R, W = 96, 256
    lin = torch.linspace(0, 1, R)
    z, y, x = torch.meshgrid(lin, lin, lin, indexing='ij')
    blob = torch.minimum(torch.sqrt((x - .45) ** 2 + (y - .5) ** 2 + (z - .5) ** 2) - 0.25,
                         torch.sqrt((x - .68) ** 2 + (y - .42) ** 2 + (z - .55) ** 2) - 0.12)
    grid = dsdf.SdfGrid(blob.float().cuda())
    sens = dsdf.get_regular_cameras(6, resx=W, resy=W)[1:4]
    seeds = [7, 8, 9]
    st = {m: dsdf.new_stats('cuda') for m in ('all', 'empty', 'none')}
    a = dsdf.render_forward(grid, sens, spp, seeds=seeds, stats=st['all'])
    b = dsdf.render_forward(grid, sens, spp, seeds=seeds, stats=st['empty'], empty_space_skip='empty-only')
    c = dsdf.render_forward(grid, sens, spp, seeds=seeds, stats=st['none'], empty_space_skip=False)
    d = {m: dsdf.stats_dict(v) for m, v in st.items()}
    assert d['all']['hits'] == d['empty']['hits'] == d['none']['hits'] > 0
    assert rel_l2(a.cpu(), b.cpu()) < 1e-6 and rel_l2(a.cpu(), c.cpu()) < 1e-6
    if spp < 16:
        # below 16 samples per pixel (HIT_PROOF_MIN_SPP, csrc/dsdf_kernels.hip) the proof costs more than the marching it saves: not computed
        assert d['all']['lanes'] == d['empty']['lanes'] and d['all']['all_steps'] == d['empty']['all_steps']
    else:
        # (deep pixels -- whole +-4 neighbourhood proven -- are not even sampled: fewer generated lanes, their samples counted as hits)
        assert d['all']['lanes'] < d['empty']['lanes']
        assert d['all']['all_steps'] < 0.9 * d['empty']['all_steps'], (d['all']['all_steps'], d['empty']['all_steps'])
    # simple shading needs the hit distance: identical step counts with and without the flag
    sa, sb = dsdf.new_stats('cuda'), dsdf.new_stats('cuda')
    e = dsdf.render_forward(grid, sens, spp, seeds=seeds, integrator=O.SIMPLE_SHADING, stats=sa)
    f = dsdf.render_forward(grid, sens, spp, seeds=seeds, integrator=O.SIMPLE_SHADING, stats=sb, empty_space_skip='empty-only')
    assert dsdf.stats_dict(sa)['all_steps'] == dsdf.stats_dict(sb)['all_steps'] and rel_l2(e.cpu(), f.cpu()) < 1e-6
    # the gradient pass is untouched by the proof (it needs the warp of every traced sample)
    gi = torch.randn(3, W, W, 3, device='cuda')
    ga = dsdf.render_backward(grid, sens, spp, gi, seeds=seeds)
    gb = dsdf.render_backward(grid, sens, spp, gi, seeds=seeds, empty_space_skip='empty-only')
    assert rel_l2(ga.cpu(), gb.cpu()) < 1e-5


@pytest.mark.parametrize('name', ['sphere64', 'blob64_flat', 'rag_x3'])
def test_device_proof_flags_match_host_proof(dsdf, harness, name):
    """The flags the device computes (k_pixel_skip + the wave-cooperative k_pixel_hit_fine, read back through the buffer of
    dsdf_share_pixel_skip) against the serial host form of the same proofs (dsdf_proof.h through tests/harness) -- and every pixel
    the DEVICE flags 'all samples hit' / 'empty' against rays traced by the host build of the march.  rag_x3 (51 x 19 x 23, tests/cases.py):
    partial last blocks on every axis of the 8^3 / 4^3 minima and the 2^3 maxima; its film is fine enough for the hit proof."""
    import ctypes as C
    from test_proof_host import _grids, PX_EMPTY, PX_HIT, RAGGED_FILMS
    from cases import RAGGED, ragged_grid
    from dsdf import _lib
    if name in RAGGED:
        grid_np = ragged_grid(RAGGED[name][0], RAGGED[name][-1]).float().numpy()
        W, H = RAGGED_FILMS[name][0]
    else:
        grid_np = _grids()[name]
        W = H = 176
    icam = 2
    origin = O.regular_camera_origins(5)[icam]
    cam = O.Camera(origin).params()
    sensor = dsdf.Sensor(origin, resx=W, resy=H)
    grid = dsdf.SdfGrid(torch.from_numpy(grid_np).cuda())
    lib = _lib.load()
    buf = torch.zeros((H + 4) * (W + 4), dtype=torch.uint8, device='cuda')
    _lib.check(lib.dsdf_share_pixel_skip(C.c_void_p(buf.data_ptr()), buf.numel()))
    try:
        dsdf.render_forward(grid, sensor, 64, seeds=[3])
    finally:
        lib.dsdf_share_pixel_skip(None, 0)
    dev = buf.cpu().numpy().reshape(H + 4, W + 4)
    host, info = harness.pixel_proof(grid_np, cam, W, H)
    assert info[1] > 0 and info[3] > 0
    d_hit, h_hit = (dev & PX_HIT) != 0, (host & PX_HIT) != 0
    d_emp, h_emp = (dev & PX_EMPTY) != 0, (host & PX_EMPTY) != 0
    assert d_hit.sum() > 0.9 * h_hit.sum() and (d_hit != h_hit).sum() <= 0.01 * h_hit.sum(), (d_hit.sum(), h_hit.sum(), (d_hit != h_hit).sum())
    assert (d_emp != h_emp).sum() <= 0.002 * h_emp.sum()
    hits = harness.trace_hits(grid_np, cam, W, H, spp=6, seed=21)
    assert hits[d_hit].all() and not hits[d_emp].any()


def test_maximum_grid_size_512(dsdf):
    """BASELINE.json's largest grid (512^3 = 537 MB padded): indexing stays in range, and the image
    of an analytic sphere agrees with the same sphere sampled at 128^3 (the half-voxel convention shifts
    the surface by 1/(2R), so the agreement is within the edge pixels)."""
    sens = dsdf.get_regular_cameras(4, resx=96, resy=96)[:2]
    imgs = {}
    for R in (128, 512):
        lin = torch.linspace(0, 1, R, device='cuda')
        z, y, x = torch.meshgrid(lin, lin, lin, indexing='ij')
        data = (torch.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2) - 0.3).contiguous()
        del x, y, z
        g = dsdf.SdfGrid(data)
        imgs[R] = dsdf.render_forward(g, sens, 64, seeds=[1, 2], integrator=O.SIMPLE_SHADING)
        if R == 512:
            gi = torch.ones(2, 96, 96, 3, device='cuda') / (96 * 96)
            grad = dsdf.render_backward(g, sens, 64, gi, seeds=[3, 4])
            assert grad.shape == (512, 512, 512) and torch.isfinite(grad).all() and float(grad.abs().sum()) > 0
            # growing the sphere (sdf -> sdf - eps) brightens the silhouette: dL/dsdf sums to a negative number
            assert float(grad.sum()) < 0
            del grad
        del g, data
        torch.cuda.empty_cache()
    assert rel_l2(imgs[512].cpu(), imgs[128].cpu()) < 0.05
    assert 0.05 < float(imgs[512].mean()) < 0.5


@pytest.mark.parametrize('integ', [O.SILHOUETTE, O.SIMPLE_SHADING])
def test_translation_parity_gpu(dsdf, integ):
    """`SamplingIntegrator.sdf.p` (python/shapes.py:389, 412, 471): image and both gradients with a
    non-zero grid translation against the oracle's autograd."""
    case = make_case('blob32')
    shift = [0.03, -0.02, 0.015]
    cam16 = case['cam'].params()

    def oracle(dt):
        data = case['grid'].to(dt).clone().requires_grad_(True)
        p = torch.tensor(shift, dtype=dt, requires_grad=True)
        ref = O.render(O.Grid3d(data, p), O.Camera.from_params(cam16, dtype=dt), case['W'], case['H'], case['spp'],
                       case['offsets'].to(dt), integ)
        (ref * case['grad_image'].to(dt)).sum().backward()
        return ref.detach(), data.grad, p.grad
    (ref, gdata, gp_ref), (_, tol_d, tol_p) = P.torch_gate(oracle)
    grid = dev_grid(dsdf, case).set_translation(shift)
    img = dsdf.render_forward(grid, sensor(dsdf, case), case['spp'], offsets=case['offsets'].cuda(), integrator=integ)[0]
    assert rel_l2(img.cpu(), ref) < FWD_TOL
    gp = torch.zeros(3, device='cuda')
    gg = dsdf.render_backward(grid, sensor(dsdf, case), case['spp'], case['grad_image'].cuda()[None],
                              offsets=case['offsets'].cuda(), integrator=integ, grad_p=gp)
    assert rel_l2(gg.cpu(), gdata) < tol_d, (rel_l2(gg.cpu(), gdata), tol_d)
    assert rel_l2(gp.cpu(), gp_ref) < tol_p, (rel_l2(gp.cpu(), gp_ref), tol_p)
    # accumulation, like grad_grid
    dsdf.render_backward(grid, sensor(dsdf, case), case['spp'], case['grad_image'].cuda()[None],
                         offsets=case['offsets'].cuda(), integrator=integ, grad_p=gp)
    assert rel_l2(gp.cpu(), 2 * gp_ref) < tol_p


@pytest.mark.parametrize('integ', [O.SILHOUETTE, O.SIMPLE_SHADING])
def test_translation_gradient_vs_finite_differences_gpu(dsdf, integ):
    """The reference's forward-gradient validation differentiates with respect to a translation
    (figures/result_utils.py:126-161); here dL/d(sdf.p) from the autograd op against central
    differences of the un-reparameterised render with common random numbers, 2048 spp, around a
    non-zero translation (same sphere scene as the data-gradient check above)."""
    R, W, H, spp = 64, 48, 48, 2048
    p0 = [0.05, -0.04, 0.03]
    data = O.sphere_grid(R, radius=0.3).float().cuda()
    sens = dsdf.get_regular_cameras(3, resx=W, resy=H)
    yy, xx = torch.meshgrid(torch.arange(H, device='cuda'), torch.arange(W, device='cuda'), indexing='ij')
    G = torch.stack([xx / W, yy / H, (xx + yy) / (W + H)], -1).float()[None].repeat(3, 1, 1, 1).contiguous()
    p = torch.tensor(p0, device='cuda', requires_grad=True)
    grid = dsdf.SdfGrid(data)
    img = dsdf.render(data, grid, sens, spp=4, seed=1, spp_grad=spp, seed_grad=11, integrator=integ, p=p)
    (img * G).sum().backward()
    assert p.grad is not None and p.grad.shape == (3,)

    def L(shift):
        g = dsdf.SdfGrid(data).set_translation(shift)
        return float((dsdf.render_forward(g, sens, spp, seeds=[11, 12, 13], integrator=integ, reparam=False) * G).sum())
    eps = 2e-3
    fds = []
    for a in range(3):
        lo, hi = list(p0), list(p0)
        lo[a] -= eps
        hi[a] += eps
        fds.append((L(hi) - L(lo)) / (2 * eps))
    ad = [float(v) for v in p.grad]
    scale = max(abs(v) for v in fds)
    # 10 %: the shading term's interior gradient has a visible estimator bias at 64^3 / 48^2 (measured 9 % on one
    # axis); the implementation itself is pinned to the oracle's autograd by test_translation_parity_gpu
    assert all(abs(x - y) < 0.10 * scale + 1.0 for x, y in zip(ad, fds)), (ad, fds)


@pytest.mark.parametrize('integ', [O.SILHOUETTE, O.SIMPLE_SHADING])
def test_forward_mode_gpu(dsdf, integ):
    """`render_forward` (integrators/reparam.py:192-196): (i) against forward-over-reverse autograd of the oracle for a
    translation tangent (the reference's eval_forward_gradient, figures/result_utils.py:126-161), (ii) transpose
    identity <J dtheta, G> == <dtheta, J^T G> with the GPU backward for tangents on sdf.data and sdf.p, several views."""
    case = make_case('sphere16')
    cam = case['cam']
    tp = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)

    def oracle(dt):
        c = O.Camera.from_params(cam.params(), dtype=dt)

        def f(p):
            return O.render(O.Grid3d(case['grid'].to(dt), p), c, case['W'], case['H'], case['spp'], case['offsets'].to(dt), integ)
        return (torch.autograd.functional.jvp(f, torch.zeros(3, dtype=dt), tp.to(dt))[1],)
    (ref,), (tol,) = P.torch_gate(oracle)
    out, img = dsdf.render_forward_grad(dev_grid(dsdf, case), sensor(dsdf, case), case['spp'], tangent_p=tp,
                                        offsets=case['offsets'].cuda(), integrator=integ, return_image=True)
    assert rel_l2(out[0].cpu(), ref) < tol, (rel_l2(out[0].cpu(), ref), tol)
    assert rel_l2(img[0].cpu(), oracle_forward(case, integ)[0]) < FWD_TOL

    case = make_case('blob48_rect')
    grid = dev_grid(dsdf, case)
    sens = dsdf.get_regular_cameras(12, resx=case['W'], resy=case['H'])[3:6]
    G = torch.randn(3, case['H'], case['W'], 3, device='cuda')
    tdata = torch.randn(grid.shape, device='cuda')
    tpv = torch.tensor([0.3, -0.7, 0.5])
    gp = torch.zeros(3, device='cuda')
    gg = dsdf.render_backward(grid, sens, 64, G, seeds=[4, 5, 6], integrator=integ, grad_p=gp)
    jd = dsdf.render_forward_grad(grid, sens, 64, tangent_data=tdata, seeds=[4, 5, 6], integrator=integ)
    jp = dsdf.render_forward_grad(grid, sens, 64, tangent_p=tpv, seeds=[4, 5, 6], integrator=integ)
    lhs_d, rhs_d = float((jd.double() * G).sum()), float((gg.double() * tdata).sum())
    lhs_p, rhs_p = float((jp.double() * G).sum()), float((gp.cpu().double() * tpv.double()).sum())
    assert abs(lhs_d - rhs_d) < 2e-3 * max(abs(rhs_d), 1.0), (lhs_d, rhs_d)
    assert abs(lhs_p - rhs_p) < 2e-3 * max(abs(rhs_p), 1.0), (lhs_p, rhs_p)
    with pytest.raises(dsdf.DsdfError):
        dsdf.render_forward_grad(grid, sens, 64, seeds=[4, 5, 6], integrator=integ)           # no tangent


def test_autograd_render_op_edge_cases(dsdf, monkeypatch):
    """What the eager schedule of the render op must survive: a second backward of the same graph (the lent queue is
    gone: the sweep is traced again), a grid update between forward and backward (refused: the queue belongs to the old grid),
    two renders outstanding at once (a queue each), and DSDF_EAGER_SWEEP=0 (plain gradient pass in backward) giving the same
    gradient."""
    case = make_case('blob32')
    data = case['grid'].float().cuda().requires_grad_(True)
    grid = dsdf.SdfGrid(data)
    sen = sensor(dsdf, case)
    w = torch.rand(1, case['H'], case['W'], 3, device='cuda')
    img = dsdf.render(data, grid, [sen], spp=64, seed=3, spp_grad=64, seed_grad=11)
    (g1,) = torch.autograd.grad((img * w).sum(), data, retain_graph=True)
    (g2,) = torch.autograd.grad((img * w).sum(), data)                 # second backward: re-traced into a private workspace
    assert g1.abs().sum() > 0 and rel_l2(g2.cpu(), g1.cpu()) < 1e-5
    # ... and the op's OTHER accumulators: dL/dp and dL/d(albedo) of a second backward start from zero again -- they are
    # not first + second -- and what the first backward returned is not written to by the second
    pt = torch.zeros(3, device='cuda', requires_grad=True)
    alb = (torch.rand(4, 4, 4, 3, device='cuda') * 0.6 + 0.2).requires_grad_(True)
    sh = dsdf.Shading(alb, 1.5, hide_emitters=True)
    imd = dsdf.render(data, grid, [sen], spp=64, seed=3, spp_grad=64, seed_grad=11, p=pt, integrator='sdf_direct_reparam', shading=sh)
    wd = torch.rand_like(imd)
    gd1, gp1, ga1 = torch.autograd.grad((imd * wd).sum(), (data, pt, alb), retain_graph=True)
    kp, ka = gp1.clone(), ga1.clone()
    gd2, gp2, ga2 = torch.autograd.grad((imd * wd).sum(), (data, pt, alb))
    assert torch.equal(gp1, kp) and torch.equal(ga1, ka)                              # the first results are untouched
    assert gp1.abs().sum() > 0 and ga1.abs().sum() > 0
    assert rel_l2(gp2.cpu(), gp1.cpu()) < 1e-4 and rel_l2(ga2.cpu(), ga1.cpu()) < 1e-5 and rel_l2(gd2.cpu(), gd1.cpu()) < 1e-5
    # two renders before one backward
    ia = dsdf.render(data, grid, [sen], spp=64, seed=3, spp_grad=64, seed_grad=11)
    ib = dsdf.render(data, grid, [sen], spp=64, seed=4, spp_grad=64, seed_grad=12)
    (gab,) = torch.autograd.grad((ia * w).sum() + (ib * w).sum(), data)
    (gb,) = torch.autograd.grad((dsdf.render(data, grid, [sen], spp=64, seed=4, spp_grad=64, seed_grad=12) * w).sum(), data)
    assert rel_l2((gab - gb).cpu(), g1.cpu()) < 1e-4
    # the lazy schedule
    monkeypatch.setenv('DSDF_EAGER_SWEEP', '0')
    (g3,) = torch.autograd.grad((dsdf.render(data, grid, [sen], spp=64, seed=3, spp_grad=64, seed_grad=11) * w).sum(), data)
    monkeypatch.delenv('DSDF_EAGER_SWEEP')
    assert rel_l2(g3.cpu(), g1.cpu()) < 1e-5
    # a grid update between forward and backward
    img = dsdf.render(data, grid, [sen], spp=64, seed=3, spp_grad=64, seed_grad=11)
    grid.update(data.detach() + 0.01)
    with pytest.raises(dsdf.DsdfError, match='updated'):
        (img * w).sum().backward()
    grid.update(data.detach())


def test_two_stream_step_equals_sequential(dsdf):
    """dsdf.render_step (primal pass and gradient sweep on two HIP streams, backward after both) == render_forward +
    render_backward: same image, same dL/dsdf (atomic-order noise), repeated to exercise the workspace hand-over."""
    case = make_case('blob48_rect')
    grid = dev_grid(dsdf, case)
    sens = dsdf.get_regular_cameras(12, resx=case['W'], resy=case['H'])[:3]
    tgt = torch.rand(3, case['H'], case['W'], 3, device='cuda')
    lg = lambda im: 2.0 * (im - tgt)
    for it in range(3):
        seeds, seeds_g = [10 * it + i for i in range(3)], [100 + 10 * it + i for i in range(3)]
        for integ in (O.SILHOUETTE, O.SIMPLE_SHADING):
            ga, gb = torch.zeros(grid.shape, device='cuda'), torch.zeros(grid.shape, device='cuda')
            ia = dsdf.render_step(grid, sens, 64, 64, lg, ga, seeds, seeds_g, integrator=integ, overlap=True)
            ib = dsdf.render_step(grid, sens, 64, 64, lg, gb, seeds, seeds_g, integrator=integ, overlap=False)
            torch.cuda.synchronize()
            assert rel_l2(ia.cpu(), ib.cpu()) < 1e-6 and rel_l2(ga.cpu(), gb.cpu()) < 1e-5


def test_shared_pixel_skip_flags(dsdf, monkeypatch):
    """dsdf_share_pixel_skip: inside dsdf.render_step the gradient sweep writes the empty-space flags and the primal render reads
    them -- same image and dL/dsdf as without sharing and as the sequential step, at a size where the proof is active, and after
    the grid changed between two steps (the flags of the previous grid must not survive the bracket)."""
    import bench
    data = bench.synth_grid(128, torch.device('cuda'))
    grid = dsdf.SdfGrid(data)
    sens = dsdf.get_regular_cameras(12, resx=192, resy=192)[2:5]
    tgt = torch.rand(3, 192, 192, 3, device='cuda')
    lg = lambda im: 2.0 * (im - tgt)
    traced = []
    for skip in (True, False):
        stats = dsdf.new_stats('cuda')
        dsdf.render_forward(grid, sens, 64, seeds=[1, 2, 3], stats=stats, empty_space_skip=skip)
        traced.append(dsdf.stats_dict(stats)['bbox_lanes'])
    assert traced[0] < 0.9 * traced[1]                                 # the proof removes work here
    for it in range(2):
        if it == 1:                                                     # another shape in the same buffers
            data = torch.roll(data, 9, dims=2).contiguous()
            grid.update(data)
        seeds, seeds_g = [5 + it, 6 + it, 7 + it], [50 + it, 60 + it, 70 + it]
        out = []
        for share, overlap in (('1', True), ('0', True), ('1', False)):
            monkeypatch.setenv('DSDF_SHARE_SKIP', share)
            g = torch.zeros(grid.shape, device='cuda')
            img = dsdf.render_step(grid, sens, 64, 64, lg, g, seeds, seeds_g, overlap=overlap)
            torch.cuda.synchronize()
            out.append((img.cpu(), g.cpu()))
        for img, g in out[1:]:
            assert rel_l2(out[0][0], img) < 1e-6 and rel_l2(out[0][1], g) < 1e-5
    # a call outside a bracket runs its own proof
    a = dsdf.render_forward(grid, sens, 64, seeds=[1, 2, 3])
    b = dsdf.render_forward(grid, sens, 64, seeds=[1, 2, 3], empty_space_skip=False)
    assert rel_l2(a.cpu(), b.cpu()) < 1e-6
