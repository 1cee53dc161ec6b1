"""The two per-sample film primitives of csrc/dsdf_math.h on their own (host build, tests/harness): the 4x4 footprint of the radius-2
Gaussian (film_taps / film_taps_each), on which every splat and gather is written, and the pair reproject_adjoint /
reproject_tangent.  The other host tests compare whole images and gradients at fp32 gates; a footprint that drifts in a border case
or an adjoint that is not the transpose of its tangent can hide under those."""
import ctypes as C

import numpy as np

from cases import make_case

BORDER, RADIUS = 2, 2.0
BIAS = float(np.float32(3.3546262790251185e-4))            # DSDF_FILTER_BIAS as the code holds it
EPS = 2.0 ** -24


def _film_taps(h, uv, Wb, Hb):
    uv = np.ascontiguousarray(uv, np.float32)
    n = len(uv)
    x0y0, w, pix = np.zeros((n, 2), np.int32), np.zeros((n, 4, 4), np.float32), np.zeros((n, 4, 4), np.int32)
    h.lib.hh_film_taps(C.c_long(n), h._p(uv), Wb, Hb, h._p(x0y0), h._p(w), h._p(pix))
    return x0y0, w, pix


def test_film_footprint(harness):
    """x0, y0 and the clipped-tap mask (with the pixel index handed to the tap body) exactly, weights within 4 x 2^-24 absolute (one
    expf, one subtract and one clamp on values <= 1), derivatives within 8 times that (one more multiply by |4 r| <= 8), against
    numpy fp64 evaluated at pos_f = uv + border - 0.5 rounded to fp32 as the code rounds it.  6 x 5 film, 10 x 9 block."""
    W, H = 6, 5
    Wb, Hb = W + 2 * BORDER, H + 2 * BORDER
    named = [
        (2.3, 1.7), (3.9, 2.2),                                        # interior
        (2.5, 1.5), (0.5, 3.5), (2.5, 2.25), (-1.5, 2.0),              # pos_f - 2 an integer on one or both axes: the ceilf tie
        (-1.3, 2.1), (-0.01, 1.0), (-2.0, 2.6), (6.0, 1.2), (7.99, 3.3),    # u in [-2, 0) and [W, W + 2): taps in the border pixels
        (-1.3, 2.1), (7.4, 2.1), (3.3, -1.2), (3.3, 6.1),              # clipped on the left / right / top / bottom block edge
        (-1.7, -1.6), (7.6, 6.4), (-1.2, 6.3), (7.3, -1.9),            # ... and in the four corners
        (-5.0, 2.0), (20.0, 20.0),                                     # no tap inside the block
    ]
    rng = np.random.default_rng(7)
    uv = np.concatenate([np.array(named), rng.uniform([-2.5, -2.5], [W + 2.5, H + 2.5], (300, 2))]).astype(np.float32)
    x0y0, w, pix = _film_taps(harness, uv, Wb, Hb)
    pf = uv + np.float32(BORDER - 0.5)                                  # fp32, like the code
    o = np.ceil(pf - np.float32(RADIUS)).astype(np.int64)
    assert np.array_equal(x0y0, o)
    q = o[:, None, :] + np.arange(4)[None, :, None]                     # (n, tap, axis) pixel coordinates
    okx, oky = (q[..., 0] >= 0) & (q[..., 0] < Wb), (q[..., 1] >= 0) & (q[..., 1] < Hb)
    inside = oky[:, :, None] & okx[:, None, :]                          # [n, j, i]
    index = q[:, :, None, 1] * Wb + q[:, None, :, 0]
    assert np.array_equal(pix, np.where(inside, index, -1))
    assert inside[:2].all() and not inside[-302:-300].any() and 0 < inside[11].sum() < 16
    r = q.astype(np.float64) - pf.astype(np.float64)[:, None, :]
    e = np.exp(-2.0 * r * r)
    f = np.maximum(0.0, e - BIAS)
    df = np.where(np.abs(r) < RADIUS, -4.0 * r * e, 0.0)
    ref = np.stack([f[..., 0], f[..., 1], df[..., 0], df[..., 1]], 1)   # wx, wy, dwx, dwy
    err_w, err_d = np.abs(w[:, :2] - ref[:, :2]).max(), np.abs(w[:, 2:] - ref[:, 2:]).max()
    print(f'footprint: weights {err_w:.3e} (bound {4 * EPS:.3e}), derivatives {err_d:.3e} (bound {32 * EPS:.3e})')
    assert err_w <= 4 * EPS and err_d <= 32 * EPS
    tie = uv[2]                                                        # the tie opens the window AT pos_f - 2: that tap has weight 0
    assert x0y0[2, 0] == tie[0] + 1.5 - 2 and w[2, 0, 0] == 0 and w[2, 2, 0] == 0


def test_reproject_adjoint_is_transpose_of_tangent(harness):
    """<reproject_adjoint(u_bar, v_bar, rw_bar), d_dir> == u_bar d_u + v_bar d_v + rw_bar d_rw (reproject_tangent) for 1000 random
    points around the blob32 camera, inside and outside its field of view and in front of its near plane.  Both sides summed in
    fp64 from the fp32 outputs; no path from an input to either scalar has more than 32 roundings, so they agree within
    32 x 2^-24 x the sum of the absolute products of a side (the smaller of the two sums is used)."""
    case = make_case('blob32')
    cam = case['cam'].params()
    n = 1000
    rng = np.random.default_rng(3)
    z = rng.uniform(0.3, 3.0, n)
    z[:50] = rng.uniform(0.002, 0.009, 50)                              # closer than near_clip: not inside
    xy = rng.uniform(-1.6, 1.6, (n, 2)) * float(cam[12]) * z[:, None]   # up to 1.6 x the half width of the film: about 60 % not inside
    R = np.stack([cam[3:6], cam[6:9], cam[9:12]], 1).astype(np.float64)
    p = (cam[0:3].astype(np.float64) + np.concatenate([xy, z[:, None]], 1) @ R.T).astype(np.float32)
    bars = rng.standard_normal((n, 3)).astype(np.float32)
    d_dir = rng.standard_normal((n, 3)).astype(np.float32)
    dir_bar, duvw, inside = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
    harness.lib.hh_reproject_pair(harness._p(cam), C.byref(harness.params), case['W'], case['H'], C.c_long(n), harness._p(p),
                                  harness._p(bars), harness._p(d_dir), harness._p(dir_bar), harness._p(duvw), harness._p(inside))
    assert 200 < inside.sum() < 800 and not inside[:50].any()
    assert (duvw[inside == 0, 2] == 0).all() and (duvw[inside == 1, 2] != 0).all()
    pl, pr = dir_bar.astype(np.float64) * d_dir, bars.astype(np.float64) * duvw
    gap = np.abs(pl.sum(1) - pr.sum(1))
    scale = np.minimum(np.abs(pl).sum(1), np.abs(pr).sum(1))
    worst = float((gap / scale).max())
    print(f'transpose: worst gap / sum of absolute products {worst:.3e} = {worst / EPS:.2f} x 2^-24 (bound 32)')
    assert (gap <= 32 * EPS * scale).all()
