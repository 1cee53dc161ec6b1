"""The film reductions of the persistent render kernels (csrc/dsdf_film.h: film_reduce_mfma -- the window sums of a 64-sample chunk
of the primal as one 16 x 16 x 4 f32 MFMA product; film_accum_wave<2> in the gradient sweep) and the items they serve
(csrc/dsdf_items_body.h).  What can go wrong here is a
layout or a bookkeeping error -- a window entry in the wrong lane or register, a clipped border, a chunk counted twice -- which is
O(1), not O(rounding): small shapes are enough.  Scene: a 24^3 grid with one sphere, two views of a 20 x 12 film (film block
24 x 16: the 5 x 5 windows are clipped on all four sides), explicit seeded offsets."""
import numpy as np
import pytest
import torch

import sdf_oracle as O
import precision as P
from conftest import rel_l2

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4            # image gate of the GPU parity tests
NCAM, ICAMS = 6, (1, 4)
W, H, R = 20, 12, 24
WB, HB = W + 4, H + 4


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    assert torch.cuda.is_available()
    return m


def sphere_grid():
    lin = torch.linspace(0, 1, R, dtype=torch.float64)
    z, y, x = torch.meshgrid(lin, lin, lin, indexing='ij')
    return (torch.sqrt((x - .5) ** 2 + (y - .5) ** 2 + (z - .5) ** 2) - 0.3).float().double()


_cases = {}


def view_case(icam, spp, w=W, h=H):
    """A tests/cases.py dict for one view of the scene (cached: the oracle's results are cached by name)."""
    key = (icam, spp, w, h)
    if key not in _cases:
        gen = torch.Generator().manual_seed(1000 * icam + spp + w)
        origin = O.regular_camera_origins(NCAM)[icam]
        _cases[key] = dict(name=f'film_reduce_v{icam}_spp{spp}_{w}x{h}', grid=sphere_grid(), ncam=NCAM, icam=icam, origin=origin,
                           cam=O.Camera(origin).rounded(), W=w, H=h, spp=spp,
                           offsets=torch.rand((w + 4) * (h + 4) * spp, 2, generator=gen, dtype=torch.float32),
                           grad_image=torch.randn(h, w, 3, generator=gen, dtype=torch.float32))
    return _cases[key]


def scene(dsdf, spp):
    cases = [view_case(i, spp) for i in ICAMS]
    grid = dsdf.SdfGrid(cases[0]['grid'].float().cuda())
    sens = [dsdf.get_regular_cameras(NCAM, resx=W, resy=H)[i] for i in ICAMS]
    offsets = torch.cat([c['offsets'] for c in cases]).cuda()
    return cases, grid, sens, offsets


def weight_sums_fp64(offsets, nv, spp):
    """fp64 weight channel of the film blocks: sample (r0, r1) of block pixel (px, py) adds g(i - 1.5 - r0) g(j - 1.5 - r1) to block
    pixel (px - 2 + i, py - 2 + j), g(x) = max(0, exp(-2 x^2) - exp(-8))."""
    r = offsets.double().numpy().reshape(nv, HB, WB, spp, 2)

    def g(x):
        return np.maximum(0.0, np.exp(-2.0 * x * x) - np.exp(-8.0))
    out = np.zeros((nv, HB, WB))
    for j in range(5):
        gy = g(j - 1.5 - r[..., 1])
        for i in range(5):
            s = (g(i - 1.5 - r[..., 0]) * gy).sum(-1)               # (nv, HB, WB): what pixel (px, py) sends to (px - 2 + i, py - 2 + j)
            dx, dy = i - 2, j - 2
            ys, yd = slice(max(0, -dy), HB - max(0, dy)), slice(max(0, dy), HB - max(0, -dy))
            xs, xd = slice(max(0, -dx), WB - max(0, dx)), slice(max(0, dx), WB - max(0, -dx))
            out[:, yd, xd] += s[:, ys, xs]
    return out


@pytest.mark.parametrize('spp', [64, 128, 256])
def test_weight_channel_against_fp64(dsdf, spp):
    """Channel 1 of EVERY film-block pixel against the fp64 sum of the window weights.  Bound: relative error 256 * 2^-24 per pixel --
    the derived worst case is 171 units in the last place (2 x 2 ulp of v_exp_f32 in the two factors, 3 roundings of the products,
    64 chain terms, at most 100 atomic adds of positive terms), rounded up to the next power of two.  The smallest fp64 weight of the
    block is that of a corner pixel, far above zero, so the relative bound applies everywhere."""
    cases, grid, sens, offsets = scene(dsdf, spp)
    film = dsdf.new_film(len(sens), W, H, dsdf.DSDF_SILHOUETTE, 'cuda')
    dsdf.render_film(grid, sens, spp, film, (0, HB), offsets=offsets, empty_space_skip=False)
    ref = weight_sums_fp64(torch.cat([c['offsets'] for c in cases]), len(sens), spp)
    got = film[..., 1].double().cpu().numpy()
    assert ref.min() > 1.0
    err = np.abs(got - ref) / ref
    print(f"spp {spp}: max relative error of the weight channel {err.max():.3e} (bound {256 * 2.0 ** -24:.3e}), min weight {ref.min():.2f}")
    assert err.max() <= 256 * 2.0 ** -24


@pytest.mark.parametrize('integ', [O.SILHOUETTE, O.SIMPLE_SHADING])
@pytest.mark.parametrize('spp', [64, 256])
def test_image_and_gradient_against_oracle(dsdf, spp, integ):
    """Primal image, gradient-pass image and dL/dsdf of both views against the fp64 C oracle, with the gates of tests/test_gpu_parity.py."""
    for icam in ICAMS:
        case = view_case(icam, spp)
        grid = dsdf.SdfGrid(case['grid'].float().cuda())
        sens = dsdf.get_regular_cameras(NCAM, resx=W, resy=H)[icam]
        ref = P.c_forward(case, integ, True)[0]
        img = dsdf.render_forward(grid, sens, spp, offsets=case['offsets'].cuda(), integrator=integ)[0]
        assert rel_l2(img.cpu(), ref) < FWD_TOL
        gg, img_g = dsdf.render_backward(grid, sens, spp, case['grad_image'].cuda()[None], offsets=case['offsets'].cuda(),
                                         integrator=integ, return_image=True)
        assert rel_l2(img_g[0].cpu(), ref) < FWD_TOL
        ok, msg = P.check_gradient('film_reduce', case, integ, True, gg.cpu().numpy())
        print(msg)
        assert ok, msg


@pytest.mark.parametrize('spp', [128, 256])
def test_proven_pixels(dsdf, spp):
    """The proofs change no result and the statistics still count every chunk: same image and the same hits with all proofs, with the
    empty-space proof alone and with none; without proofs every block sample is generated; the scene holds traced, hit-proven,
    empty and deep pixels (the three step totals differ, fewer lanes with the hit proof than without).
    On the 24^3 / 20 x 12 scene of this file no level of the min-grids covers the spread of a pixel's rays (csrc/dsdf_proof.h:
    skip_level returns -1 -- a pixel is wider than a voxel), so no pixel is ever proven there: all three modes gave the same
    98 304 lanes, 13 910 hits and 534 999 steps at spp 128.  The same sphere is therefore rendered at the voxel-to-pixel ratio of
    test_hit_proof_is_exact (96^3 grid, 256 x 256 film), where every pixel class occurs -- which the assertions below check."""
    R2, W2 = 96, 256
    lin = torch.linspace(0, 1, R2, dtype=torch.float64)
    z, y, x = torch.meshgrid(lin, lin, lin, indexing='ij')
    grid = dsdf.SdfGrid((torch.sqrt((x - .5) ** 2 + (y - .5) ** 2 + (z - .5) ** 2) - 0.3).float().cuda())
    sens = [dsdf.get_regular_cameras(NCAM, resx=W2, resy=W2)[i] for i in ICAMS]
    gen = torch.Generator(device='cuda').manual_seed(spp)
    offsets = torch.rand(len(sens) * (W2 + 4) * (W2 + 4) * spp, 2, generator=gen, device='cuda', dtype=torch.float32)
    st, img = {}, {}
    for mode in (True, 'empty-only', False):
        stats = dsdf.new_stats('cuda')
        img[mode] = dsdf.render_forward(grid, sens, spp, offsets=offsets, stats=stats, empty_space_skip=mode).cpu()
        st[mode] = dsdf.stats_dict(stats)
    print({str(m): {k: st[m][k] for k in ('lanes', 'hits', 'all_steps')} for m in st})
    assert rel_l2(img[True], img['empty-only']) < 1e-6 and rel_l2(img[True], img[False]) < 1e-6
    assert st[True]['hits'] == st['empty-only']['hits'] == st[False]['hits'] > 0
    assert st[False]['lanes'] == len(sens) * (W2 + 4) * (W2 + 4) * spp
    assert st[True]['lanes'] < st[False]['lanes'] and st[True]['lanes'] % 64 == 0
    steps = [st[m]['all_steps'] for m in (True, 'empty-only', False)]
    assert len(set(steps)) == 3, steps
    assert st[True]['lanes'] < st['empty-only']['lanes']


def test_row_windows(dsdf):
    """Two row windows of the film block accumulated into one film equal the full-height call: the flush's bounds test and the work
    list's row window."""
    spp = 128
    cases, grid, sens, offsets = scene(dsdf, spp)
    whole = dsdf.new_film(len(sens), W, H, dsdf.DSDF_SILHOUETTE, 'cuda')
    dsdf.render_film(grid, sens, spp, whole, (0, HB), offsets=offsets)
    parts = dsdf.new_film(len(sens), W, H, dsdf.DSDF_SILHOUETTE, 'cuda')
    for rows in ((0, 7), (7, HB)):
        dsdf.render_film(grid, sens, spp, parts, rows, offsets=offsets)
    assert rel_l2(parts.cpu(), whole.cpu()) < 1e-6
    assert rel_l2(dsdf.develop(parts, W, H).cpu(), dsdf.develop(whole, W, H).cpu()) < 1e-6


@pytest.mark.parametrize('integ', [O.SILHOUETTE, O.SIMPLE_SHADING])
def test_ragged_film(dsdf, integ):
    """A 19 x 13 film (block 23 x 17: partial work-list tiles), one view, spp 64, against the oracle."""
    case = view_case(ICAMS[0], 64, 19, 13)
    grid = dsdf.SdfGrid(case['grid'].float().cuda())
    sens = dsdf.get_regular_cameras(NCAM, resx=19, resy=13)[ICAMS[0]]
    ref = P.c_forward(case, integ, True)[0]
    img = dsdf.render_forward(grid, sens, 64, offsets=case['offsets'].cuda(), integrator=integ)[0]
    assert rel_l2(img.cpu(), ref) < FWD_TOL
    gg, img_g = dsdf.render_backward(grid, sens, 64, case['grad_image'].cuda()[None], offsets=case['offsets'].cuda(),
                                     integrator=integ, return_image=True)
    assert rel_l2(img_g[0].cpu(), ref) < FWD_TOL
    ok, msg = P.check_gradient('film_reduce', case, integ, True, gg.cpu().numpy())
    assert ok, msg
