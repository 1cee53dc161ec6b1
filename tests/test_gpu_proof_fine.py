"""The second stage of the empty-space proof on the device (k_pixel_hit_fine over the full-resolution window minima, bit 7 =
DSDF_PX_EMPTY_FINE and more of bit 1; csrc/dsdf_skip.h) against its stand-alone host build, and the renders with the stage on and
off (empty_space_skip='coarse-empty' = DSDF_NO_FINE_EMPTY): the stage is a proof, so images, gradients, hit counts and the backward
queue stay what they were and only marching steps disappear.  Cases: those of
test_gpu_parity.py::test_device_proof_flags_match_host_proof."""
import ctypes as C

import pytest
import torch

import sdf_oracle as O
from conftest import rel_l2
from proof_fine_cases import CASES, ICAM, NCAM, PX_EMPTY, PX_EMPTY_FINE, PX_EMPTY_G, PX_HIT, case, host_flags

pytestmark = pytest.mark.gpu
OFF = 'coarse-empty'


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    assert torch.cuda.is_available()
    return m


def _scene(dsdf, name):
    grid_np, W, H, origin = case(name)
    return dsdf.SdfGrid(torch.from_numpy(grid_np).cuda()), dsdf.Sensor(origin, resx=W, resy=H), W, H


def _shared_flags(dsdf, grid, sensor, W, H, **kw):
    from dsdf import _lib
    lib = _lib.load()
    buf = torch.zeros((H + 4) * (W + 4), dtype=torch.uint8, device='cuda')
    _lib.check(lib.dsdf_share_pixel_skip(C.c_void_p(buf.data_ptr()), buf.numel()))
    try:
        dsdf.render_forward(grid, sensor, 64, seeds=[3], **kw)
    finally:
        lib.dsdf_share_pixel_skip(None, 0)
    return buf.cpu().numpy().reshape(H + 4, W + 4)


@pytest.mark.parametrize('name', CASES)
def test_fine_flags_match_host_and_leave_bits_0_and_4(dsdf, harness, name):
    """Bits 0 and 4 of the shared buffer are byte-equal with the stage on and off (they keep meaning 'proven by the block bounds', which
    test_device_proof_flags_match_host_proof compares with a host build that has no fine stage); bits 7 and 1 match the host build of the
    fine stage up to centre-ray rounding: 0.2 % of the coarse-proven pixels, the allowance of that test."""
    grid, sensor, W, H = _scene(dsdf, name)
    on = _shared_flags(dsdf, grid, sensor, W, H)
    off = _shared_flags(dsdf, grid, sensor, W, H, empty_space_skip=OFF)
    keep = PX_EMPTY | PX_HIT
    assert ((on & keep) == (off & keep)).all()
    assert not (off & PX_EMPTY_FINE).any()
    assert not ((on & PX_EMPTY_FINE) != 0)[(on & PX_HIT) != 0].any()
    coarse, fine, info = host_flags(harness, name)
    h_emp, h_g = (fine & PX_EMPTY) != 0, (fine & PX_EMPTY_G) != 0
    d_emp, d_g = (on & (PX_EMPTY | PX_EMPTY_FINE)) != 0, (on & PX_EMPTY_G) != 0
    base = int(((coarse & PX_EMPTY) != 0).sum())
    n7, n1 = int((d_emp != h_emp).sum()), int((d_g != h_g).sum())
    print(f"{name}: device bit 7 on {int(((on & PX_EMPTY_FINE) != 0).sum())} pixels; primal-empty device {int(d_emp.sum())} host {int(h_emp.sum())} "
          f"mismatch {n7}; gradient-empty device {int(d_g.sum())} host {int(h_g.sum())} mismatch {n1}; allowance {0.002 * base:.1f}")
    assert ((on & PX_EMPTY_FINE) != 0).sum() > 0 and d_g.sum() > ((off & PX_EMPTY_G) != 0).sum()
    assert n7 <= 0.002 * base and n1 <= 0.002 * base, (n7, n1, base)


def _pair(dsdf, grid, sens, spp, integrator, seeds, gi, **kw):
    """(image, gradient, forward stats, backward stats) of one forward + backward render, for the stage on and off."""
    out = {}
    for mode in (True, OFF):
        sf, sb = dsdf.new_stats('cuda'), dsdf.new_stats('cuda')
        img = dsdf.render_forward(grid, sens, spp, seeds=seeds, integrator=integrator, stats=sf, empty_space_skip=mode, **kw)
        gg = dsdf.render_backward(grid, sens, spp, gi, seeds=seeds, integrator=integrator, stats=sb, empty_space_skip=mode, **kw)
        out[mode] = (img.cpu(), gg.cpu(), dsdf.stats_dict(sf), dsdf.stats_dict(sb))
    return out[True], out[OFF]


def _same_result_fewer_steps(a, b, what):
    (img_a, gg_a, fa, ba), (img_b, gg_b, fb, bb) = a, b
    print(f"{what}: forward all_steps {fa['all_steps']} vs {fb['all_steps']} (off), backward {ba['all_steps']} vs {bb['all_steps']}, "
          f"hits {fa['hits']}, queue_len {ba['queue_len']}, image rel-L2 {rel_l2(img_a, img_b):.2e}, gradient {rel_l2(gg_a, gg_b):.2e}")
    assert rel_l2(img_a, img_b) < 1e-6 and rel_l2(gg_a, gg_b) < 1e-5
    assert fa['hits'] == fb['hits'] > 0 and ba['hits'] == bb['hits']
    assert ba['queue_len'] == bb['queue_len']
    assert fa['all_steps'] < fb['all_steps'] and ba['all_steps'] < bb['all_steps']


@pytest.mark.parametrize('integ', [O.SILHOUETTE, O.SIMPLE_SHADING])
@pytest.mark.parametrize('name', CASES)
def test_renders_agree_with_and_without_the_fine_stage(dsdf, name, integ):
    grid, sensor, W, H = _scene(dsdf, name)
    gi = torch.randn(1, H, W, 3, generator=torch.Generator().manual_seed(5)).cuda()
    a, b = _pair(dsdf, grid, sensor, 64, integ, [7], gi)
    _same_result_fewer_steps(a, b, f"{name} integrator {integ}")


def test_direct_with_a_visible_environment(dsdf):
    """sdf_direct_reparam, environment visible: the film pixels only proven-empty pixels reach get the environment from k_film_env, whose
    mask now counts bit 7 -- on a 16^3 sphere, whose two 8^3 blocks per axis leave the block minima nothing to prove, under a film fine
    enough for the fine stage."""
    W = H = 176
    grid = dsdf.SdfGrid(O.sphere_grid(16).float().cuda())
    sens = dsdf.get_regular_cameras(NCAM, resx=W, resy=H)[ICAM]
    gen = torch.Generator().manual_seed(9)
    sh = dsdf.Shading((torch.rand(3, 4, 5, 3, generator=gen) * 0.6 + 0.2).cuda(), (1.0, 0.9, 0.8), hide_emitters=False)
    gi = torch.randn(1, H, W, 3, generator=gen).cuda()
    a, b = _pair(dsdf, grid, sens, 64, 'sdf_direct_reparam', [11], gi, shading=sh)
    _same_result_fewer_steps(a, b, 'direct, visible environment')


def test_lane_pass_reads_the_fine_flags(dsdf):
    """spp 4: k_render_pass, one lane per sample, reads the same flags."""
    grid, sensor, W, H = _scene(dsdf, 'sphere64')
    gi = torch.randn(1, H, W, 3, generator=torch.Generator().manual_seed(6)).cuda()
    a, b = _pair(dsdf, grid, sensor, 4, O.SILHOUETTE, [8], gi)
    _same_result_fewer_steps(a, b, 'sphere64 spp 4')


def test_render_step_shares_the_fine_flags(dsdf):
    """One step through the shared bracket (dsdf_share_pixel_skip): the first call's proof writes bits 7 and 1 for both passes."""
    grid, sensor, W, H = _scene(dsdf, 'blob64_flat')
    sens = [sensor, dsdf.Sensor(O.regular_camera_origins(NCAM)[0], resx=W, resy=H)]
    w = torch.randn(2, H, W, 3, generator=torch.Generator().manual_seed(4)).cuda()
    res = {}
    for mode in (True, OFF):
        gg = torch.zeros(grid.rz, grid.ry, grid.rx, device='cuda')
        img = dsdf.render_step(grid, sens, 64, 64, lambda im: w, gg, [1, 2], [3, 4], empty_space_skip=mode)
        torch.cuda.synchronize()
        res[mode] = (img.cpu(), gg.cpu())
    e_img, e_g = rel_l2(res[True][0], res[OFF][0]), rel_l2(res[True][1], res[OFF][1])
    print(f"render_step: image rel-L2 {e_img:.2e}, gradient {e_g:.2e}")
    assert e_img < 1e-6 and e_g < 1e-5 and float(res[True][1].abs().sum()) > 0
