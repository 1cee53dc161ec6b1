"""Shared by tests/test_proof_value_host.py and tests/test_gpu_proof_value.py: the stand-alone host build of the third proof stage
(tests/harness/dsdf_proof_stages_host.cpp: spline value on the centre ray -+ a gradient bound, csrc/dsdf_proof.h) on the cases of
tests/proof_fine_cases.py plus one grid of plain random values, which is no SDF."""
import ctypes as C
import functools

import numpy as np

import sdf_oracle as O
import proof_fine_cases as F

from proof_fine_cases import PX_EMPTY, PX_EMPTY_FINE, PX_EMPTY_G, PX_HIT, PX_KEEP, _p, host_lib

NOISE = 'noise64'
CASES = F.CASES + [NOISE]


@functools.lru_cache(None)
def case(name):
    """(grid (Z,Y,X) float32, W, H, camera origin) of one case."""
    if name == NOISE:
        # plain random values: neighbouring taps differ by up to 0.6 where an SDF of this resolution changes by 1 / 64 per voxel, so
        # the gradient bound is some forty times an SDF's and the stage must prove next to nothing -- and still be right
        grid = np.random.default_rng(7).uniform(-0.1, 0.5, (64, 64, 64)).astype(np.float32)
        return grid, 176, 176, O.regular_camera_origins(F.NCAM)[F.ICAM]
    return F.case(name)


_flags = {}


def device_camera(name):
    """The float32[16] camera record the DEVICE receives for the case's sensor: dsdf.Sensor's own look-at frame, rounded to fp32 when it
    fills the C struct -- not the oracle's Camera.params()."""
    import dsdf
    _, W, H, origin = case(name)
    c = dsdf.Sensor(origin, resx=W, resy=H).to_struct()
    return np.array(list(c.origin) + list(c.left) + list(c.up) + list(c.dir) + [c.tan_half_fov, 0, 0, 0], np.float32)


def host_flags(harness, name, want_hit=True, cam=None):
    """dict(coarse, two, merged, third, info): block-bound flags of the host harness (its hit proof on the block maxima only), then per
    listed pixel what the second stage adds in its two-loop and its merged form and what the third stage proves, in the encoding of the
    flag byte (bit 7 / 1 / 4).  info = (step, r, D_x, D_y, D_z).  cam: another float32[16] camera record than the oracle's for the case.
    Computed once per case and camera, shared by the tests, never modified."""
    key = (name, bool(want_hit), None if cam is None else cam.tobytes())
    if key not in _flags:
        grid, W, H, origin = case(name)
        cam = np.ascontiguousarray(O.Camera(origin).params() if cam is None else cam, np.float32)
        coarse, _ = harness.pixel_proof(grid, cam, W, H, stages=1 if want_hit else 0)
        coarse = np.ascontiguousarray(coarse)
        rz, ry, rx = grid.shape
        two, merged, third = (np.zeros((H + 4, W + 4), np.uint8) for _ in range(3))
        info = np.zeros(4, np.float32)
        step = host_lib().psh_proofs(_p(grid), rx, ry, rz, C.byref(harness.params), _p(cam), W, H, _p(coarse), int(want_hit), _p(two), _p(merged),
                                     _p(third), _p(info))
        assert step > 0
        out = dict(coarse=coarse, two=two, merged=merged, third=third, info=(float(step),) + tuple(float(v) for v in info))
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _flags[key] = out
    return _flags[key]


def trace(params, name, spp, seed, mask):
    """(H+4, W+4, spp) uint8 for the pixels of `mask`: bit 0 = the sample hits in the primal's march, bit 1 = in the differentiable march,
    bit 2 = its boundary weight is positive."""
    grid, W, H, origin = case(name)
    cam = np.ascontiguousarray(O.Camera(origin).params(), np.float32)
    rz, ry, rx = grid.shape
    out = np.zeros((H + 4, W + 4, spp), np.uint8)
    mask = np.ascontiguousarray(mask, np.uint8)
    host_lib().psh_trace(_p(grid), rx, ry, rz, C.byref(params), _p(cam), W, H, spp, C.c_uint(seed), _p(mask), _p(out))
    return out


def dilate(keep):
    """Bits 2 / 3 / 5 / 6 of k_skip_dilate from the KEEP bits of a (Hb, Wb) plane."""
    Hb, Wb = keep.shape
    emp = ((keep & (PX_EMPTY | PX_EMPTY_FINE)) != 0)
    bits = {4: emp, 8: (keep & PX_EMPTY_G) != 0, 32: (keep & PX_HIT) != 0, 64: (keep & PX_HIT) != 0}
    out = np.zeros_like(keep)
    for bit, m in bits.items():
        r = 2 if bit == 64 else 4
        p = np.pad(m, r, constant_values=True)
        acc = np.ones_like(m)
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                acc &= p[dy:dy + Hb, dx:dx + Wb]
        out |= np.where(acc, bit, 0).astype(np.uint8)
    return out
