"""Inputs, reference, bounds and the residual check shared by the redistancing tests (test_redistance_host.py, test_gpu_redistance.py).

All fields are sampled at the voxel centres of the unit cube, (i + 0.5) / res per axis, and are fp32 arrays of shape (Z, Y, X).
The reference is the fp64 build of the C oracle (oracle/dsdf_oracle.c: o_redistance), computed once per input and shared."""
import functools

import numpy as np

RD_TILE = 8          # csrc/dsdf_redistance.h: DSDF_RD_TILE
RD_TOL = 1e-5        # csrc/dsdf_redistance.h: DSDF_RD_TOL (voxels of the x spacing)
RD_BIG = 1e10        # csrc/dsdf_eikonal.h: DSDF_RD_BIG, the value of a voxel that no front reaches


def centres(shape):
    return np.meshgrid(*[(np.arange(s) + 0.5) / s for s in shape], indexing='ij')       # z, y, x


def _factor(x, y, z):
    return 1.5 + 0.5 * np.sin(7 * x + 3 * y) * np.cos(5 * z)        # smooth, in [1, 2]: phi is no distance field, its zero set is kept


def corner_sphere(shape, radius=0.08):
    """Distorted sphere about the grid corner (0, 0, 0): the front runs through the whole grid and distances grow to about 1.7.
    Non-cubic shapes take the anisotropic update."""
    z, y, x = centres(shape)
    return ((np.sqrt(x * x + y * y + z * z) - radius) * _factor(x, y, z)).astype(np.float32)


def corner_circle(shape, radius=0.08):
    """The same about the z axis through the corner, for grids one or two voxels deep (their voxel centres lie farther than
    `radius` from the corner itself): hz >> hx = hy, the anisotropic update."""
    z, y, x = centres(shape)
    return ((np.sqrt(x * x + y * y) - radius) * _factor(x, y, z)).astype(np.float32)


def centred_sphere(shape, radius=0.3):
    z, y, x = centres(shape)
    return ((np.sqrt((x - .5) ** 2 + (y - .45) ** 2 + (z - .55) ** 2) - radius) * _factor(x, y, z)).astype(np.float32)


def spheres_and_slab(shape):
    """Two spheres and a slab about one voxel thick that runs into the grid boundary."""
    z, y, x = centres(shape)
    a = np.sqrt((x - .3) ** 2 + (y - .3) ** 2 + (z - .25) ** 2) - 0.12
    b = np.sqrt((x - .7) ** 2 + (y - .65) ** 2 + (z - .8) ** 2) - 0.1
    s = np.abs(z - 0.5 + 0.1 * x) - 0.6 / shape[0]
    return (np.minimum(np.minimum(a, b), s) * _factor(x, y, z)).astype(np.float32)


def random_normal(shape, seed=0):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def single_zero(shape=(9, 10, 11)):
    phi = np.ones(shape, np.float32)
    phi[4, 5, 6] = 0.0
    return phi


@functools.lru_cache(maxsize=None)
def _phi(kind, shape, sign):
    phi = sign * {'corner': corner_sphere, 'circle': corner_circle, 'centred': centred_sphere, 'slab': spheres_and_slab, 'normal': random_normal,
                  'zero': single_zero, 'ones': lambda s: np.ones(s, np.float32)}[kind](shape)
    phi = np.ascontiguousarray(phi, np.float32)
    phi.setflags(write=False)
    return phi


@functools.lru_cache(maxsize=None)
def _ref(kind, shape, sign):
    import c_oracle
    ref = c_oracle.redistance(c_oracle.load(double=True), _phi(kind, shape, sign))
    ref.setflags(write=False)
    return ref


def case(kind, shape, sign=1):
    """(phi fp32, fp64-oracle result) of a named input; both read-only and computed once per session."""
    return _phi(kind, tuple(shape), sign), _ref(kind, tuple(shape), sign)


def spacings(shape):
    rz, ry, rx = shape
    return 1.0 / rx, 1.0 / ry, 1.0 / rz


def ulp32(v):
    return float(np.spacing(np.float32(v)))


def finite(ref):
    """The voxels some front reaches (an input without an interface leaves every voxel at +-DSDF_RD_BIG)."""
    return np.abs(ref) < RD_BIG


def host_bound(ref):
    """Bound on max |fp32 result - fp64 oracle| in absolute units: 4 (rx + ry + rz) ulp32(max |ref|).  A well-conditioned update
    loses a few ulp OF THE VALUE'S MAGNITUDE per grid step, and a causal chain is at most the grid's Manhattan length."""
    rz, ry, rx = ref.shape
    f = finite(ref)
    return 4.0 * (rx + ry + rz) * ulp32(np.abs(ref[f]).max() if f.any() else 1.0)


def gpu_bound(ref):
    """host_bound + the deferral the re-activation tolerance permits: a face value that moved by <= DSDF_RD_TOL h does not
    wake the neighbour tile, once per tile crossing of a causal chain (at most ntx + nty + ntz crossings)."""
    rz, ry, rx = ref.shape
    nt = sum((r + RD_TILE - 1) // RD_TILE for r in (rx, ry, rz))
    return host_bound(ref) + nt * RD_TOL / rx


def ntiles(shape):
    return int(np.prod([(r + RD_TILE - 1) // RD_TILE for r in shape]))


def frozen_mask(phi):
    """Voxels the initialisation freezes: exact zeros and voxels whose sign differs from a 6-neighbour's."""
    pos = phi > 0
    fz = phi == 0
    for ax in range(3):
        d = np.swapaxes(pos, 0, ax)[1:] != np.swapaxes(pos, 0, ax)[:-1]
        m = np.zeros_like(np.swapaxes(pos, 0, ax))
        m[1:] |= d
        m[:-1] |= d
        fz = fz | np.swapaxes(m, 0, ax)
    return fz


def godunov_residual(out, phi):
    """max over the non-frozen voxels of |u - G(neighbours of u)| in fp64, G the Godunov upwind solution of |grad u| = 1 from the
    6 neighbours (vectorised): zero exactly at the scheme's fixed point, whatever order of updates led there."""
    u = np.abs(np.asarray(out, np.float64))
    hx, hy, hz = spacings(u.shape)
    pad = np.pad(u, 1, constant_values=RD_BIG)
    nb = [np.minimum(pad[1:-1, 1:-1, :-2], pad[1:-1, 1:-1, 2:]), np.minimum(pad[1:-1, :-2, 1:-1], pad[1:-1, 2:, 1:-1]),
          np.minimum(pad[:-2, 1:-1, 1:-1], pad[2:, 1:-1, 1:-1])]
    v = np.stack(nb); h = np.broadcast_to(np.array([hx, hy, hz]).reshape(3, 1, 1, 1), v.shape)
    order = np.argsort(v, axis=0)
    v = np.take_along_axis(v, order, 0); h = np.take_along_axis(h, order, 0)
    w = 1.0 / (h * h)
    p, r = v[1] - v[0], v[2] - v[0]                         # (differences from the smallest neighbour: exact enough in fp64)
    with np.errstate(invalid='ignore', over='ignore'):
        t1 = h[0]
        A2, B2, C2 = w[0] + w[1], -2 * w[1] * p, w[1] * p * p - 1
        t2 = (-B2 + np.sqrt(np.maximum(B2 * B2 - 4 * A2 * C2, 0))) / (2 * A2)
        A3, B3, C3 = A2 + w[2], -2 * (w[1] * p + w[2] * r), w[1] * p * p + w[2] * r * r - 1
        t3 = (-B3 + np.sqrt(np.maximum(B3 * B3 - 4 * A3 * C3, 0))) / (2 * A3)
    t = np.where(t1 <= p, t1, np.where(t2 <= r, t2, t3))
    g = v[0] + t
    free = ~frozen_mask(phi) & (v[0] < RD_BIG)
    return float(np.abs(u - g)[free].max()) if free.any() else 0.0
