"""Shared by tests/test_gpu_grid_buffer.py and tests/test_proof_fine_host.py: small noise grids, the layout of the library's grid
buffer written out from the table in include/dsdf.h (dsdf_padded_size), and every array of it by numpy brute force.  min, max and one
fp32 subtraction round the same way everywhere, so all of it compares with ==."""
import functools

import numpy as np

GRIDS = [(2, 2, 2), (4, 5, 6), (9, 8, 7), (17, 16, 33)]          # (rx, ry, rz)
MIN_SHIFTS, HIT_SHIFT, HIT_RADIUS = (3, 2), 1, 2


@functools.lru_cache(None)
def noise(dims):
    """(rz, ry, rx) float32 of seeded uniform noise in [-0.3, 0.7], read-only."""
    rx, ry, rz = dims
    g = np.random.default_rng(1000 * rx + 100 * ry + rz).uniform(-0.3, 0.7, (rz, ry, rx)).astype(np.float32)
    g.setflags(write=False)
    return g


def blocks(dims, shift):
    rx, ry, rz = dims
    return tuple(-(-r >> shift) for r in (rz, ry, rx))


def layout(dims):
    """name -> (offset in floats, shape) of every array of the buffer, and the total."""
    rx, ry, rz = dims
    out, n = {}, 0

    def take(name, shape):
        nonlocal n
        out[name] = (n, shape)
        n += int(np.prod(shape))
    take('padded', (rz + 6, ry + 6, rx + 6))
    for level, shift in enumerate(MIN_SHIFTS):
        take(f'min_raw{level}', blocks(dims, shift))
        take(f'min_dil{level}', blocks(dims, shift))
    take('max_raw', blocks(dims, HIT_SHIFT))
    take('max_dil', blocks(dims, HIT_SHIFT))
    take('win_max', (rz, ry, rx))
    take('win_min', (rz, ry, rx))
    n = (n + 3) // 4 * 4
    take('rows', ((rx + 2) // 4 + 1, rz + 6, ry + 6, 8))
    return out, n


def _fold_shifts(p, shape, span, maxi):
    """min / max over the span^3 shifted windows of shape `shape` in p."""
    f, out = (np.maximum if maxi else np.minimum), None
    for dz in range(span):
        for dy in range(span):
            for dx in range(span):
                s = p[dz:dz + shape[0], dy:dy + shape[1], dx:dx + shape[2]]
                out = s.copy() if out is None else f(out, s)
    return out


def block_bounds(grid, shift, radius, maxi):
    """(raw, dilated): min / max over blocks of (1 << shift)^3 voxels, then over the blocks within `radius`."""
    C, fill = 1 << shift, np.float32(-np.inf if maxi else np.inf)
    nb = [-(-r >> shift) for r in grid.shape]
    p = np.pad(grid, [(0, b * C - r) for b, r in zip(nb, grid.shape)], constant_values=fill)
    p = p.reshape(nb[0], C, nb[1], C, nb[2], C)
    raw = p.max((1, 3, 5)) if maxi else p.min((1, 3, 5))
    return raw, _fold_shifts(np.pad(raw, radius, constant_values=fill), raw.shape, 2 * radius + 1, maxi)


def window(grid, maxi):
    """min / max over the taps [c - 2, c + 3]^3, clamped to the grid (an edge value repeated changes neither)."""
    return _fold_shifts(np.pad(grid, (2, 3), mode='edge'), grid.shape, 6, maxi)


@functools.lru_cache(None)
def reference(dims):
    """name -> array for the arrays of layout() a test may assert (the raw block arrays are scratch), plus 'D' (3 floats at the start
    of max_raw, or None: fewer than three such blocks).  Computed once per grid, read-only."""
    rx, ry, rz = dims
    g = noise(dims)
    ref = {'padded': np.pad(g, 3, mode='edge'), 'max_dil': block_bounds(g, HIT_SHIFT, HIT_RADIUS, True)[1],
           'win_max': window(g, True), 'win_min': window(g, False)}
    for level, shift in enumerate(MIN_SHIFTS):
        ref[f'min_dil{level}'] = block_bounds(g, shift, 1, False)[1]
    xs = np.minimum(4 * np.arange((rx + 2) // 4 + 1)[:, None] + np.arange(8)[None, :], rx + 5)            # (xc, k) -> padded x
    ref['rows'] = np.ascontiguousarray(ref['padded'][:, :, xs].transpose(2, 0, 1, 3))
    ref['D'] = None
    if int(np.prod(blocks(dims, HIT_SHIFT))) >= 3:
        ref['D'] = np.array([np.abs(np.diff(g, axis=ax)).max() if g.shape[ax] > 1 else 0 for ax in (2, 1, 0)], np.float32)
    for v in ref.values():
        if v is not None:
            v.setflags(write=False)
    return ref
