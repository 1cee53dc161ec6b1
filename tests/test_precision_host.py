"""The set-aside of single-sample flips in image comparisons (tests/precision.py image_rel_l2_but_flips) must not hide real errors."""
import numpy as np

import precision as P


def _image(H=40, W=48, seed=0):
    rng = np.random.default_rng(seed)
    img = np.zeros((H, W, 3))
    img[8:30, 10:38] = rng.uniform(0.2, 1.0, 3)                      # a lit object on black, value range ~1
    return img


def _splat(img, y, x, amp):
    """The change of one flipped sample: amp x the 4 x 4 Gaussian footprint around (y, x)."""
    out = img.copy()
    w = np.exp(-((np.arange(4) - 1.5) ** 2) / (2 * 0.25))
    out[y - 1:y + 3, x - 1:x + 3] += amp * np.outer(w, w)[..., None]
    return out


def test_one_flip_is_set_aside():
    ref = _image()
    spp = 64
    img = _splat(ref, 20, 20, 1.0 / spp)
    plain, rest, windows = P.image_rel_l2_but_flips(img, ref, 1e-4, spp)
    assert plain > 1e-4 and rest < 1e-4 and len(windows) == 1
    assert windows[0]['removed'] <= windows[0]['bound']


def test_errors_that_are_not_one_flip_are_kept():
    ref = _image()
    spp = 64
    # larger than any one sample can move
    plain, rest, windows = P.image_rel_l2_but_flips(_splat(ref, 20, 20, 8.0 / spp), ref, 1e-4, spp)
    assert rest == plain and windows == []
    # a flip-sized error at the film border
    plain, rest, windows = P.image_rel_l2_but_flips(_splat(ref, 1, 20, 1.0 / spp), ref, 1e-4, spp)
    assert rest == plain and windows == []
    # on env-filled pixels of sdf_direct_reparam
    env = (1.0, 0.9, 0.8)
    ref_env = np.where((ref == 0).all(-1, keepdims=True), np.asarray(env), ref)
    plain, rest, windows = P.image_rel_l2_but_flips(_splat(ref_env, 35, 40, 1.0 / spp), ref_env, 1e-4, spp, env=env)
    assert rest == plain and windows == []
    plain, rest, windows = P.image_rel_l2_but_flips(_splat(ref_env, 20, 20, 1.0 / spp), ref_env, 1e-4, spp, env=env)
    assert rest < 1e-4 and len(windows) == 1
    # at most two windows
    img = _splat(_splat(_splat(ref, 12, 14, 1.0 / spp), 20, 24, 1.0 / spp), 26, 32, 1.0 / spp)
    plain, rest, windows = P.image_rel_l2_but_flips(img, ref, 1e-4, spp)
    assert len(windows) == 2 and rest > 1e-4
