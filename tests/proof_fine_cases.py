"""Shared by tests/test_proof_fine_host.py and tests/test_gpu_proof_fine.py: the cases of the device-flag test
(test_gpu_parity.py::test_device_proof_flags_match_host_proof) and the stand-alone host build of the second stage of the
empty-space proof and of the third proof stage (tests/harness/dsdf_proof_stages_host.cpp; tests/proof_value_cases.py uses the same
library and constants)."""
import ctypes as C
import functools

import numpy as np

import sdf_oracle as O
from host_build import ptr as _p, shared_lib

CASES = ['sphere64', 'blob64_flat', 'rag_x3']
PX_EMPTY, PX_EMPTY_G, PX_HIT, PX_EMPTY_FINE = 1, 2, 16, 128
PX_KEEP = PX_EMPTY | PX_EMPTY_G | PX_HIT | PX_EMPTY_FINE
ICAM, NCAM = 2, 5


@functools.lru_cache(None)
def host_lib():
    lib = shared_lib('dsdf_proof_stages_host.cpp')
    lib.psh_fine_empty.restype = lib.psh_proofs.restype = C.c_float
    return lib


@functools.lru_cache(None)
def case(name):
    """(grid (Z,Y,X) float32, W, H, camera origin) of one case."""
    from cases import RAGGED, ragged_grid
    from test_proof_host import _grids, RAGGED_FILMS
    if name in RAGGED:
        grid = ragged_grid(RAGGED[name][0], RAGGED[name][-1]).float().numpy()
        W, H = RAGGED_FILMS[name][0]
    else:
        grid = _grids()[name]
        W = H = 176
    return np.ascontiguousarray(grid, np.float32), W, H, O.regular_camera_origins(NCAM)[ICAM]


def fine_empty(params, grid, cam, W, H):
    """flags (H+4, W+4) of pixel_empty_proof over the window minima (bits 0 / 1 as that function returns them), and its step."""
    rz, ry, rx = grid.shape
    flags = np.zeros((H + 4, W + 4), np.uint8)
    cam = np.ascontiguousarray(cam, np.float32)
    step = host_lib().psh_fine_empty(_p(grid), rx, ry, rz, C.byref(params), _p(cam), W, H, _p(flags))
    return flags, float(step)


def sample_weights(params, grid, cam, W, H, spp, seed, mask):
    """(H+4, W+4, spp) uint8 for the pixels of `mask`: bit 0 = the sample hits, bit 1 = its boundary weight is positive."""
    rz, ry, rx = grid.shape
    out = np.zeros((H + 4, W + 4, spp), np.uint8)
    cam = np.ascontiguousarray(cam, np.float32)
    mask = np.ascontiguousarray(mask, np.uint8)
    host_lib().psh_trace(_p(grid), rx, ry, rz, C.byref(params), _p(cam), W, H, spp, C.c_uint(seed), _p(mask), _p(out))
    return out >> 1         # (psh_trace: bit 0 = the primal's march hits, then these two)


def window(grid, maxi):
    """Window minima / maxima (Z,Y,X) as the three separable passes build them."""
    rz, ry, rx = grid.shape
    out = np.zeros_like(grid)
    host_lib().psh_window(_p(grid), rx, ry, rz, int(maxi), _p(out))
    return out


def block_bounds(grid, shift, radius, maxi):
    """(raw, dilated) block minima / maxima over blocks of (1 << shift)^3 voxels, each (ceil(rz / C), ceil(ry / C), ceil(rx / C))."""
    rz, ry, rx = grid.shape
    raw, dil = (np.zeros([-(-r >> shift) for r in grid.shape], np.float32) for _ in range(2))
    host_lib().psh_block_bounds(_p(grid), rx, ry, rz, shift, radius, int(maxi), _p(raw), _p(dil))
    return raw, dil


_host_flags = {}


def host_flags(harness, name):
    """(coarse flags of the host harness, fine flags, info): computed once per case, shared by the tests, never modified."""
    if name not in _host_flags:
        grid, W, H, origin = case(name)
        cam = O.Camera(origin).params()
        coarse, info = harness.pixel_proof(grid, cam, W, H)
        fine, fstep = fine_empty(harness.params, grid, cam, W, H)
        assert fstep == info[3] > 0
        coarse.setflags(write=False); fine.setflags(write=False)
        _host_flags[name] = (coarse, fine, info)
    return _host_flags[name]
