"""The third proof stage on the device (k_pixel_hit_fine: spline value on the centre ray -+ a gradient bound, csrc/dsdf_proof.h) --
where its results go, against its stand-alone host build, and the renders with the stage on and off
(empty_space_skip='window-empty' = DSDF_NO_VALUE_BOUND).  The caller-visible flag byte must not change at all: the stage writes a
library-private effective plane (the second half of a shared buffer of two planes, or the render workspace), which the render stages
read.  The stage is a proof, so images, gradients, hit counts and the backward queue stay what they were and only marching steps
disappear.  Cases: those of tests/proof_fine_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import sdf_oracle as O
from conftest import rel_l2
from proof_fine_cases import CASES, ICAM, NCAM
from proof_value_cases import PX_EMPTY, PX_EMPTY_FINE, PX_EMPTY_G, PX_HIT, PX_KEEP, case, dilate, host_flags

pytestmark = pytest.mark.gpu
OFF = 'window-empty'


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    assert torch.cuda.is_available()
    return m


def _scene(dsdf, name):
    grid_np, W, H, origin = case(name)
    return dsdf.SdfGrid(torch.from_numpy(grid_np).cuda()), dsdf.Sensor(origin, resx=W, resy=H), W, H


def _shared_flags(dsdf, grid, sensor, W, H, planes, **kw):
    """The caller's buffer after one render inside a bracket: (planes, H+4, W+4), prefilled with 0xff."""
    from dsdf import _lib
    lib = _lib.load()
    buf = torch.full((planes * (H + 4) * (W + 4),), 255, dtype=torch.uint8, device='cuda')
    _lib.check(lib.dsdf_share_pixel_skip(C.c_void_p(buf.data_ptr()), buf.numel()))
    try:
        dsdf.render_forward(grid, sensor, 64, seeds=[3], **kw)
    finally:
        lib.dsdf_share_pixel_skip(None, 0)
    return buf.cpu().numpy().reshape(planes, H + 4, W + 4)


_dev = {}


def _device_flags(dsdf, name):
    """name -> {(planes, on): buffer}: computed once per case, shared by the tests, never modified."""
    if name not in _dev:
        grid, sensor, W, H = _scene(dsdf, name)
        _dev[name] = {(p, on): _shared_flags(dsdf, grid, sensor, W, H, p, empty_space_skip=True if on else OFF)
                      for p in (1, 2) for on in (True, False)}
        for v in _dev[name].values():
            v.setflags(write=False)
    return _dev[name]


@pytest.mark.parametrize('name', CASES)
def test_caller_visible_plane_is_unchanged(dsdf, name):
    """(a) With a one-plane and with a two-plane buffer the first plane is byte-equal with the stage on and off."""
    d = _device_flags(dsdf, name)
    ref = d[(1, False)][0]
    for key in ((1, True), (2, True), (2, False)):
        assert (d[key][0] == ref).all(), (key, int((d[key][0] != ref).sum()))
    assert (d[(2, False)][1] == 255).all(), "the stage is off: nothing may touch the second plane"


@pytest.mark.parametrize('name', CASES)
def test_effective_plane_matches_host(dsdf, harness, name):
    """(b) KEEP bits of the second plane = KEEP bits of the first plus what the host build of the stage proves, up to centre-ray rounding:
    0.2 % of the coarse-proven pixels, the allowance of tests/test_gpu_proof_fine.py; its dilated bits follow from its own KEEP bits exactly."""
    d = _device_flags(dsdf, name)
    first, plane = d[(2, True)]
    h = host_flags(harness, name, True)
    want = (first & np.uint8(PX_KEEP)) | h['third']
    base = int(((h['coarse'] & PX_EMPTY) != 0).sum())
    bad = {bit: int((((plane ^ want) & np.uint8(bit)) != 0).sum()) for bit in (PX_EMPTY, PX_EMPTY_G, PX_HIT, PX_EMPTY_FINE)}
    added = {bit: int(((plane & ~first & np.uint8(bit)) != 0).sum()) for bit in (PX_EMPTY_G, PX_HIT, PX_EMPTY_FINE)}
    print(f"{name}: the plane adds {added} to the first plane's KEEP bits; mismatches against the host build {bad}; allowance {0.002 * base:.1f}")
    assert bad[PX_EMPTY] == 0
    assert all(n > 0 for n in added.values())
    assert all(n <= 0.002 * base for n in bad.values()), (bad, base)
    assert ((plane & np.uint8(0xff ^ PX_KEEP)) == dilate(plane & np.uint8(PX_KEEP))).all()


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
def test_renders_agree_with_and_without_the_stage(dsdf, name, integ):
    """(c) stand-alone calls: the plane lives in the render workspace."""
    grid, sensor, W, H = _scene(dsdf, name)
    gi = torch.randn(1, H, W, 3, generator=torch.Generator().manual_seed(5)).cuda()
    a, b = _pair(dsdf, grid, sensor, 64, integ, [7], gi)
    _same_result_fewer_steps(a, b, f"{name} integrator {integ}")


def test_lane_pass_reads_the_plane(dsdf):
    """(c) spp 4: k_render_pass, one lane per sample, reads the same plane."""
    grid, sensor, W, H = _scene(dsdf, 'sphere64')
    gi = torch.randn(1, H, W, 3, generator=torch.Generator().manual_seed(6)).cuda()
    a, b = _pair(dsdf, grid, sensor, 4, O.SILHOUETTE, [8], gi)
    _same_result_fewer_steps(a, b, 'sphere64 spp 4')


def _planes(buf, n):
    """(first plane, second plane) of a shared buffer, n bytes each, on the host."""
    b = buf[:2 * n].cpu().numpy()
    return b[:n].copy(), b[n:].copy()


def _plane_carries_the_stage(first, plane, what):
    """The second plane is a superset of the first in every KEEP bit and holds strictly more of bits 7, 1 and 4."""
    keep = np.uint8(PX_KEEP)
    assert ((first & keep) & ~plane == 0).all()
    more = {bit: (int(((plane & np.uint8(bit)) != 0).sum()), int(((first & np.uint8(bit)) != 0).sum())) for bit in (PX_EMPTY_FINE, PX_EMPTY_G, PX_HIT)}
    print(f"{what}: pixels with bit (second plane, first plane) {more}")
    assert all(a > b for a, b in more.values()), more


SENTINEL = 0xA5


def test_render_step_shares_the_plane(dsdf):
    """(c) One step through the shared bracket (dsdf_share_pixel_skip).  render_step takes no statistics, so that the stage is ON inside
    the bracket is read from step_begin's own buffer: it must hold two planes, the sweep's proof must have written the second with
    strictly more proven pixels than the first, and the primal render reads that one.  With the stage off the second plane is not touched
    and the first is byte-equal.  Image and gradient agree."""
    from dsdf import renderer
    grid, sensor, W, H = _scene(dsdf, 'blob64_flat')
    sens = [sensor, dsdf.Sensor(O.regular_camera_origins(NCAM)[0], resx=W, resy=H)]
    n = len(sens) * (H + 4) * (W + 4)
    w = torch.randn(2, H, W, 3, generator=torch.Generator().manual_seed(4)).cuda()
    res, planes = {}, {}
    for mode in (True, OFF):
        buf = renderer._skip_buffers.get(grid.device)
        if buf is not None:
            buf.fill_(SENTINEL)
        gg = torch.zeros(grid.rz, grid.ry, grid.rx, device='cuda')
        img = dsdf.render_step(grid, sens, 64, 64, lambda im: w, gg, [1, 2], [3, 4], empty_space_skip=mode)
        torch.cuda.synchronize()
        res[mode] = (img.cpu(), gg.cpu())
        buf = renderer._skip_buffers[grid.device]
        assert buf.numel() >= 2 * n, "step_begin's buffer must hold two planes, or the stage is off for every step"
        planes[mode] = _planes(buf, n)
    _plane_carries_the_stage(*planes[True], 'render_step')
    assert (planes[OFF][1] == SENTINEL).all(), "the stage is off: nothing may touch the second plane"
    assert (planes[OFF][0] == planes[True][0]).all()
    e_img, e_g = rel_l2(res[True][0], res[OFF][0]), rel_l2(res[True][1], res[OFF][1])
    print(f"render_step: image rel-L2 {e_img:.2e}, gradient {e_g:.2e}")
    assert e_img < 1e-6 and e_g < 1e-5 and float(res[True][1].abs().sum()) > 0


def test_hip_ops_share_the_plane(dsdf):
    """The multi-GPU step's operators (parallel.HipOps, one rank): begin_group's buffer holds two planes and the stage runs in its
    bracket, as in render_step."""
    from dsdf import parallel
    grid, sensor, W, H = _scene(dsdf, 'sphere64')
    sens = [sensor, dsdf.Sensor(O.regular_camera_origins(NCAM)[0], resx=W, resy=H)]
    n = len(sens) * (H + 4) * (W + 4)
    w = torch.randn(2, H, W, 3, generator=torch.Generator().manual_seed(3)).cuda()
    res, planes = {}, {}
    for mode in (True, OFF):
        ops = parallel.HipOps(grid, sens, 64, 64, [1, 2], [3, 4], O.SILHOUETTE, empty_space_skip=mode)
        gg = torch.zeros(grid.rz, grid.ry, grid.rx, device='cuda')
        img = parallel.render_step(ops, len(sens), W, H, 0, 1, lambda im: w, gg)
        torch.cuda.synchronize()
        res[mode] = (img.cpu(), gg.cpu())
        assert ops._flags.numel() >= 2 * n, "begin_group's buffer must hold two planes, or the stage is off for every step"
        planes[mode] = _planes(ops._flags, n)
    _plane_carries_the_stage(*planes[True], 'HipOps')
    assert (planes[OFF][1] == 255).all(), "the stage is off: the second plane keeps what begin_group left there"
    assert (planes[OFF][0] == planes[True][0]).all()
    # the row balancer's cost model reads the plane the render stages read: less predicted work with the stage on, and with it off
    # exactly what the first plane alone gives
    cost = {mode: parallel.row_costs(torch.from_numpy(np.concatenate(planes[mode])).cuda(), len(sens), W + 4, H + 4, 64, 64) for mode in (True, OFF)}
    first_only = parallel.row_costs(torch.from_numpy(planes[OFF][0]).cuda(), len(sens), W + 4, H + 4, 64, 64)
    print(f"HipOps row costs: {float(cost[True].sum()):.4g} with the stage, {float(cost[OFF].sum()):.4g} without")
    assert float(cost[True].sum()) < float(cost[OFF].sum()) and torch.equal(cost[OFF], first_only)
    e_img, e_g = rel_l2(res[True][0], res[OFF][0]), rel_l2(res[True][1], res[OFF][1])
    print(f"HipOps step: image rel-L2 {e_img:.2e}, gradient {e_g:.2e}")
    assert e_img < 1e-6 and e_g < 1e-5 and float(res[True][1].abs().sum()) > 0


def test_direct_with_a_visible_environment(dsdf):
    """(d) sdf_direct_reparam, environment visible: k_film_env reads the plane -- the film pixels only proven-empty pixels reach get the
    environment -- on a 16^3 sphere under a film fine enough for the fine stages."""
    W = H = 176
    grid = dsdf.SdfGrid(O.sphere_grid(16).float().cuda())
    sens = dsdf.get_regular_cameras(NCAM, resx=W, resy=H)[ICAM]
    gen = torch.Generator().manual_seed(9)
    sh = dsdf.Shading((torch.rand(3, 4, 5, 3, generator=gen) * 0.6 + 0.2).cuda(), (1.0, 0.9, 0.8), hide_emitters=False)
    gi = torch.randn(1, H, W, 3, generator=gen).cuda()
    a, b = _pair(dsdf, grid, sens, 64, 'sdf_direct_reparam', [11], gi, shading=sh)
    _same_result_fewer_steps(a, b, 'direct, visible environment')
