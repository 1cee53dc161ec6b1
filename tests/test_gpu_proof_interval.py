"""The restricted loop of the fine proof stages on the device (k_pixel_hit_fine: csrc/dsdf_proof.h, proof_interval /
pixel_fine_proofs_near) against the host build of the same statements (tests/harness/dsdf_proof_interval_host.cpp, which
tests/test_proof_interval_host.py holds equal to the loop over the whole ray): the caller-visible flag plane and the effective plane,
byte for byte, with the hit proof on and off.  Two views at 32^2; their field of view is narrow (6 and 4 degrees, aimed at the
silhouette) because the fine stages run only where a pixel's sample rays stay within a voxel of its centre ray, and both stand at
the same distance, in coordinates fp32 holds exactly, so that the batch's margins are those of each view alone.  The host build gets
the camera records the device gets."""
import ctypes as C

import numpy as np
import pytest
import torch

import proof_interval_cases as I
from proof_value_cases import PX_EMPTY, PX_EMPTY_FINE, PX_EMPTY_G, PX_HIT, PX_KEEP, dilate

pytestmark = pytest.mark.gpu
W = H = 32
ORIGINS = [(2.0, 1.25, -0.5), (-1.0, 1.25, -0.5)]        # centre + (+-1.5, 0.75, -1)


def _sphere64():
    import sdf_oracle as O
    return np.ascontiguousarray(O.sphere_grid(64).float().numpy())


# name -> (grid, field of view, target): a point of the sphere's silhouette for both views ((0, 1, 0.75) is normal to both view
# directions); a stretch of the noise grid where one view proves about half of its pixels empty and the other none
SCENES = {'sphere64': (_sphere64, 6.0, (0.5, 0.74, 0.68)), 'noise_rag': (lambda: I.grid('noise_rag'), 4.0, (0.55, 0.6, 0.4))}


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    assert torch.cuda.is_available()
    return m


def _record(sensor):
    c = sensor.to_struct()
    return np.array(list(c.origin) + list(c.left) + list(c.up) + list(c.dir) + [c.tan_half_fov, 0, 0, 0], np.float32)


def _fine_bits(m):
    m = m.astype(np.uint8)
    return np.where(m & PX_EMPTY, PX_EMPTY_FINE, 0).astype(np.uint8) | (m & np.uint8(PX_EMPTY_G | PX_HIT))


def _device(dsdf, grid, sensors, want_hit):
    from dsdf import _lib
    lib = _lib.load()
    n = len(sensors) * (H + 4) * (W + 4)
    buf = torch.full((2 * n,), 255, dtype=torch.uint8, device='cuda')
    _lib.check(lib.dsdf_share_pixel_skip(C.c_void_p(buf.data_ptr()), buf.numel()))
    try:
        dsdf.render_forward(grid, sensors, 64, seeds=[3, 4], empty_space_skip=True if want_hit else 'empty-only')
    finally:
        lib.dsdf_share_pixel_skip(None, 0)
    return buf.cpu().numpy().reshape(2, len(sensors), H + 4, W + 4)


def _host(harness, g, cam, want_hit):
    """(flag plane, effective plane) of one view from the host build: block stage, fine stages on the pixels it lists, dilation."""
    coarse, info = harness.pixel_proof(g, cam, W, H, stages=1 if want_hit else 0)
    coarse = coarse & np.uint8(PX_EMPTY | PX_EMPTY_G | PX_HIT)
    listed = ((coarse & (PX_EMPTY | PX_HIT)) == 0) | ((coarse & 3) == PX_EMPTY)
    r = I.proofs(harness.params, g, cam, W, H, want_hit & ((coarse & PX_EMPTY) == 0), True, listed)
    first = coarse | _fine_bits(r['near'] & 0xff)
    plane = first | _fine_bits(r['near'] >> 8)
    return first | dilate(first), plane | dilate(plane), listed


@pytest.mark.parametrize('want_hit', [True, False])
@pytest.mark.parametrize('name', sorted(SCENES))
def test_device_planes_equal_the_host_build(dsdf, harness, name, want_hit):
    make, fov, target = SCENES[name]
    g = make()
    sensors = [dsdf.Sensor(o, target=target, fov=fov, resx=W, resy=H) for o in ORIGINS]
    dev = _device(dsdf, dsdf.SdfGrid(torch.from_numpy(g.copy()).cuda()), sensors, want_hit)
    for v, s in enumerate(sensors):
        first, plane, listed = _host(harness, g, _record(s), want_hit)
        d1, d2 = dev[0, v], dev[1, v]
        fine = d1 & np.uint8(PX_EMPTY_FINE)
        print(f"{name} view {v} hit proof {want_hit}: {int(listed.sum())} of {listed.size} pixels listed; device flag plane: empty "
              f"{int(((d1 & PX_EMPTY) != 0).sum())}, fine-empty {int((fine != 0).sum())}, hit {int(((d1 & PX_HIT) != 0).sum())}; the effective "
              f"plane adds KEEP bits on {int((((d2 ^ d1) & np.uint8(PX_KEEP)) != 0).sum())}; differing bytes: flag plane "
              f"{int((d1 != first).sum())}, effective plane {int((d2 != plane).sum())}")
        assert listed.sum() > 50, "the fine stages had nothing to do: the comparison would be vacuous"
        assert (d1 == first).all(), f"flag plane, view {v}: {int((d1 != first).sum())} bytes differ, first {np.argwhere(d1 != first)[:4].tolist()}"
        assert (d2 == plane).all(), f"effective plane, view {v}: {int((d2 != plane).sum())} bytes differ, first {np.argwhere(d2 != plane)[:4].tolist()}"
