"""The split backward of the one-channel integrators (dsdf_grad_sweep: k_backward_coef beside and behind the tail kernel, which also
writes the rows k_backward_apply locates a sample's scatter points with; dsdf_grad_backward: k_backward_apply with the counts of a
group and the film footprint of a sample each in one round of loads) on small films: against the fp64 oracle with the gate of
tests/test_gpu_parity.py, against the fused kernel of dsdf.render_backward, and on films and scenes that leave partial groups, empty
groups, full units and a view without a single queued sample.  (The issue's grid-stride case has no subject: the strided,
software-pipelined form of the apply kernel measured slower and was not kept)

32^3 grids, 2 views at 24 x 20 (or the ragged sizes), 64 spp in the gradient pass, image gradients with random signs.  The oracle
gradient of a multi-view call is the sum over its views (one C-oracle run per view, cached by tests/precision.py); its gate is
P.check_gradient's formula on the summed case: max(2 x the fp32 floor of the summed gradient, 1e-4)."""
import numpy as np
import pytest
import torch

import precision as P
import sdf_oracle as O

rel_l2 = P.rel_l2

pytestmark = pytest.mark.gpu

INTEGRATORS = [O.SILHOUETTE, O.SIMPLE_SHADING]
SPP = 64


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    assert torch.cuda.is_available()
    return m


_scenes = {}


def scene(tag):
    """name: (grid, W, H, cameras of the ring, views taken, seed) -> per-view case dicts as tests/cases.py builds them."""
    if tag not in _scenes:
        gridfn, W, H, ncam, icams, seed = {
            'blob': (lambda: O.blob_grid(32, n=6, seed=1), 24, 20, 3, (1, 2), 71),
            # unit count of the film block (27 x 23 = 621 pixels) no multiple of the 16 units of a group
            'ragged_film': (lambda: O.blob_grid(32, n=6, seed=1), 23, 19, 3, (0, 2), 72),
            # a small sphere in a large film: most groups queue nothing, the units on its rim queue all 64 samples
            'small_sphere': (lambda: O.sphere_grid(32, radius=0.12), 40, 28, 3, (0, 1), 73),
        }[tag]
        gen = torch.Generator().manual_seed(seed)
        grid = gridfn()
        origins = O.regular_camera_origins(ncam)
        views = []
        for icam in icams:
            offsets = torch.rand((W + 4) * (H + 4) * SPP, 2, generator=gen, dtype=torch.float32)
            grad_image = torch.randn(H, W, 3, generator=gen, dtype=torch.float32)
            views.append(dict(name=f'apply_{tag}_v{icam}', grid=grid, ncam=ncam, icam=icam, origin=origins[icam],
                              cam=O.Camera(origins[icam]).rounded(), W=W, H=H, spp=SPP, offsets=offsets, grad_image=grad_image))
        _scenes[tag] = dict(grid=grid, W=W, H=H, ncam=ncam, icams=icams, views=views)
    return _scenes[tag]


def gpu_inputs(dsdf, sc):
    grid = dsdf.SdfGrid(sc['grid'].float().cuda())
    ring = dsdf.get_regular_cameras(sc['ncam'], resx=sc['W'], resy=sc['H'])
    sens = [ring[i] for i in sc['icams']]
    offsets = torch.cat([v['offsets'] for v in sc['views']]).cuda()
    gi = torch.stack([v['grad_image'] for v in sc['views']]).cuda()
    return grid, sens, offsets, gi


def split_backward(dsdf, grid, sens, gi, integ, offsets=None, seeds=None):
    """dsdf_grad_sweep (coefficients beside the tail kernel up to the snapshot, then from it) + dsdf_grad_backward (apply)."""
    W, H = sens[0].film_size()
    sw = dsdf.GradSweep(grid, sens, SPP, (0, H + 4), seeds=seeds, offsets=offsets, integrator=integ)
    film = sw.sweep(dsdf.new_film(len(sens), W, H, integ, grid.device))
    gg = torch.zeros(grid.shape, device=grid.device)
    sw.backward(film, gi.contiguous(), gg)
    torch.cuda.synchronize()
    return gg


def check_sum_of_views(tag, views, integ, gg):
    refs = [P.reference_gradient(v, integ, True) for v in views]
    g64, g32 = sum(r['g64'] for r in refs), sum(r['g32'] for r in refs)
    floor = rel_l2(g32, g64)
    tol = max(P.FLOOR_FACTOR * floor, P.NORTH_STAR)
    e = rel_l2(gg, g64)
    print(f"{tag} integ {integ}: rel-L2 {e:.3e} vs fp32 floor {floor:.3e}, gate {tol:.3e}; |g| {np.abs(g64).sum():.3e}")
    assert np.isfinite(gg).all() and np.abs(g64).max() > 0
    assert e <= tol, (tag, integ, e, floor, tol)


@pytest.mark.parametrize('integ', INTEGRATORS)
def test_against_the_oracle(dsdf, integ):
    sc = scene('blob')
    grid, sens, offsets, gi = gpu_inputs(dsdf, sc)
    fused = dsdf.render_backward(grid, sens, SPP, gi, offsets=offsets, integrator=integ).cpu().numpy()
    check_sum_of_views('render_backward', sc['views'], integ, fused)
    split = split_backward(dsdf, grid, sens, gi, integ, offsets=offsets).cpu().numpy()
    check_sum_of_views('sweep + backward', sc['views'], integ, split)


@pytest.mark.parametrize('integ', INTEGRATORS)
def test_the_two_call_shapes_agree(dsdf, integ):
    """dsdf.render_step (the sweep with both coefficient launches, then the apply kernel) against dsdf.render_backward, to 4 x the
    relative L2 difference of two runs of render_backward itself (the order of the atomics differs between any two runs).
    (render_backward runs the fused k_backward, render_step the two halves; on MI355X two runs differ by 0.9e-7 / 1.4e-7 and the
    two call shapes by 1.0e-7 / 1.3e-7, silhouette / simple shading.)"""
    sc = scene('blob')
    grid, sens, _, gi = gpu_inputs(dsdf, sc)
    seeds, seeds_g = [3, 4], [13, 14]
    a = dsdf.render_backward(grid, sens, SPP, gi, seeds=seeds_g, integrator=integ).cpu().numpy()
    b = dsdf.render_backward(grid, sens, SPP, gi, seeds=seeds_g, integrator=integ).cpu().numpy()
    g = torch.zeros(grid.shape, device='cuda')
    dsdf.render_step(grid, sens, SPP, SPP, lambda im: gi, g, seeds, seeds_g, integrator=integ)
    torch.cuda.synchronize()
    noise, e = rel_l2(b, a), rel_l2(g.cpu().numpy(), a)
    print(f"integ {integ}: two runs of render_backward {noise:.3e}; render_step against render_backward {e:.3e}")
    assert np.abs(a).max() > 0
    assert e <= 4 * noise, (integ, e, noise)


@pytest.mark.parametrize('integ', INTEGRATORS)
@pytest.mark.parametrize('tag', ['ragged_film', 'small_sphere'])
def test_ragged_shapes(dsdf, tag, integ):
    sc = scene(tag)
    grid, sens, offsets, gi = gpu_inputs(dsdf, sc)
    split = split_backward(dsdf, grid, sens, gi, integ, offsets=offsets).cpu().numpy()
    check_sum_of_views(tag, sc['views'], integ, split)


@pytest.mark.parametrize('integ', INTEGRATORS)
def test_a_view_that_queues_nothing(dsdf, integ):
    """Two views, the second looks away from the box: its queue stays empty, the call's gradient is the first view's."""
    sc = scene('blob')
    v = sc['views'][0]
    grid, sens, _, _ = gpu_inputs(dsdf, sc)
    away = dsdf.Sensor((2.0, 1.0, 2.0), target=(4.0, 1.5, 4.0), resx=sc['W'], resy=sc['H'])
    offsets = torch.cat([v['offsets'], sc['views'][1]['offsets']]).cuda()
    gi = torch.stack([v['grad_image'], sc['views'][1]['grad_image']]).cuda()
    alone = split_backward(dsdf, grid, [away], gi[1:], integ, offsets=offsets[offsets.shape[0] // 2:]).cpu().numpy()
    assert np.abs(alone).max() == 0
    split = split_backward(dsdf, grid, [sens[0], away], gi, integ, offsets=offsets).cpu().numpy()
    check_sum_of_views('empty view', [v], integ, split)
