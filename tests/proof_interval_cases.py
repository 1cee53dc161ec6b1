"""Shared by tests/test_proof_interval_host.py, tests/test_gpu_proof_interval.py and tools/sim_proof_interval.py: the stand-alone host
build of the fine proof stages in both forms (tests/harness/dsdf_proof_interval_host.cpp) -- the reference loop over the whole centre
ray and the one restricted to the stretch near the shape (csrc/dsdf_proof.h: proof_interval, pixel_fine_proofs_near) -- and the grids
that are built to go wrong: a surface on the box faces, a slab two voxels thick, a ragged noise grid."""
import ctypes as C
import functools

import numpy as np

import sdf_oracle as O
from host_build import ptr as _p, shared_lib

COUNTERS = ['round', 'light', 'leap', 'bmin', 'bmax', 'value', 'walk']      # csrc/dsdf_proof.h: DSDF_PC_*
NOISE_SHAPE = (17, 16, 33)


@functools.lru_cache(None)
def host_lib():
    lib = shared_lib('dsdf_proof_interval_host.cpp')
    lib.psi_proofs.restype = lib.psi_certificate.restype = C.c_float
    return lib


def _axes(shape):
    """voxel-centre coordinates in [0, 1] per axis, (Z,Y,X) broadcastable"""
    rz, ry, rx = shape
    z, y, x = (((np.arange(n) + 0.5) / n) for n in (rz, ry, rx))
    return z[:, None, None], y[None, :, None], x[None, None, :]


@functools.lru_cache(None)
def grid(name):
    """(Z,Y,X) float32, read-only."""
    if name == 'halfspace64':
        # solid below z = 0.5 through the whole box: the surface and the interior reach the box faces, so a ray ENTERS at the shape
        # (ta = t0) or LEAVES in it (tb = t1)
        z, y, x = _axes((64, 64, 64))
        g = (z - 0.5) + 0 * y + 0 * x
    elif name in ('slab64', 'plate64'):
        # a tilted plate two voxels thick (slab64): every run of the hit proof is shorter than the landing bound J that the positions
        # BEFORE the interval feed, no pixel proves a hit -- with a J that is too small some would; and six voxels thick (plate64): window
        # maxima never fall below 0 on it, the third stage alone proves hits, behind that prefix
        z, y, x = _axes((64, 64, 64))
        n = np.array([0.25, 0.35, 0.9]); n /= np.linalg.norm(n)
        g = np.abs((x - 0.5) * n[0] + (y - 0.5) * n[1] + (z - 0.5) * n[2]) - (1.0 if name == 'slab64' else 3.0) / 64
        g = np.maximum(g, np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2) - 0.3)      # (a disc: rays pass beside it too)
    elif name == 'noise_rag':
        # plain random values, no SDF, ragged, two 8^3 blocks thin along y: from 0.03 up, where the thresholds of the rays lie (0.01 (t1 +
        # 0.1) 1.05: 0.02 .. 0.035), so that block minima pass for one ray and fail for the next; one pocket below 0 at the far end
        # of x, whose dilated blocks leave x < 16 alone
        rng = np.random.default_rng(11)
        g = rng.uniform(0.03, 0.6, NOISE_SHAPE)
        g[2:4, 11:14, 27:31] = rng.uniform(-0.05, 0.02, (2, 3, 4))
    else:
        raise KeyError(name)
    g = np.ascontiguousarray(g, np.float32)
    g.setflags(write=False)
    return g


def camera(i, n=5, **kw):
    return np.ascontiguousarray(O.Camera(O.regular_camera_origins(n)[i], **kw).params(), np.float32)


def proofs(params, g, cam, W, H, want_hit, third=True, listed=None):
    """dict(ref, near: uint16 (H+4, W+4), both bytes of the reference and of the restricted form; ival (.., 4): ta, tb, t0, t1;
    cnt (.., 2, len(COUNTERS)): per form; step, cstep) for the pixels of `listed` (bool, default: every pixel)."""
    rz, ry, rx = g.shape
    n = (H + 4, W + 4)
    lst = np.ones(n, np.uint8) if listed is None else np.ascontiguousarray(listed, np.uint8)
    hit = np.broadcast_to(np.asarray(want_hit, bool), n)
    lst = np.ascontiguousarray(np.where(lst != 0, 1 + 2 * hit, 0), np.uint8)
    ref, near = np.zeros(n, np.uint16), np.zeros(n, np.uint16)
    ival, cnt, info = np.zeros(n + (4,), np.float32), np.zeros(n + (2, len(COUNTERS)), np.int32), np.zeros(2, np.float32)
    cam = np.ascontiguousarray(cam, np.float32)
    step = host_lib().psi_proofs(_p(g), rx, ry, rz, C.byref(params), _p(cam), W, H, _p(lst), int(third), _p(ref), _p(near), _p(ival),
                                 _p(cnt), _p(info))
    assert step > 0, "the fine stages are off for this film, or the entry without counters disagrees with the counted one (-1)"
    return dict(ref=ref, near=near, ival=ival, cnt=cnt, step=float(step), cstep=float(info[0]), listed=lst != 0)


def window_min_brute(g):
    """(Z,Y,X) minimum over the taps clamp(c - 2 .. c + 3) per axis of cell c, from the definition."""
    rz, ry, rx = g.shape
    out = np.empty_like(g)
    for z in range(rz):
        zs = np.clip(np.arange(z - 2, z + 4), 0, rz - 1)
        for y in range(ry):
            ys = np.clip(np.arange(y - 2, y + 4), 0, ry - 1)
            for x in range(rx):
                xs = np.clip(np.arange(x - 2, x + 4), 0, rx - 1)
                out[z, y, x] = g[np.ix_(zs, ys, xs)].min()
    return out


def certificate(params, g, wmin, cam, W, H):
    """dict(min, n, thr, ival) per film-block pixel: the smallest of `wmin` over the fine positions outside [ta, tb], their number, what
    they have to exceed, (ta, tb, t0, t1)."""
    rz, ry, rx = g.shape
    n = (H + 4, W + 4)
    omin, on, thr, ival = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n + (4,), np.float32)
    cam = np.ascontiguousarray(cam, np.float32)
    wmin = np.ascontiguousarray(wmin, np.float32)
    step = host_lib().psi_certificate(_p(g), _p(wmin), rx, ry, rz, C.byref(params), _p(cam), W, H, _p(omin), _p(on), _p(thr), _p(ival))
    assert step > 0
    return dict(min=omin, n=on, thr=thr, ival=ival, step=float(step))
