"""CPU check of the SECOND stage of the empty-space proof (csrc/dsdf_proof.h: pixel_empty_proof over the full-resolution window
minima, DSDF_PX_EMPTY_FINE / more of DSDF_PX_EMPTY_G) through the stand-alone host build of the fine stages (tests/harness/dsdf_proof_stages_host.cpp),
against traced sample rays: every sample of a pixel the stage flags must miss, and -- for bit 1 -- carry a zero boundary weight.
The render kernels skip the march of such pixels, so a single counter-example here would be a wrong image or gradient.
Cases: those of test_gpu_parity.py::test_device_proof_flags_match_host_proof."""
import numpy as np
import pytest

import sdf_oracle as O
import grid_buffer_cases as B
from proof_fine_cases import CASES, PX_EMPTY, PX_EMPTY_G, block_bounds, case, host_flags, sample_weights, window

SPP = 6


def test_window_minima_are_the_6x6x6_tap_minima():
    """The three separable passes against a brute-force minimum over the taps [c - 2, c + 3]^3 (clamped to the grid)."""
    grid = case('rag_x3')[0]
    m = window(grid, False)
    rz, ry, rx = grid.shape
    rng = np.random.default_rng(0)
    pts = np.concatenate([rng.integers(0, [rz, ry, rx], (300, 3)), [[0, 0, 0], [rz - 1, ry - 1, rx - 1], [0, ry - 1, 1], [rz - 2, 0, rx - 1]]])
    for z, y, x in pts:
        ref = grid[max(z - 2, 0):z + 4, max(y - 2, 0):y + 4, max(x - 2, 0):x + 4].min()
        assert m[z, y, x] == ref, (z, y, x)


@pytest.mark.parametrize('dims', [(4, 5, 6), (9, 8, 7)])
@pytest.mark.parametrize('maxi', [False, True])
def test_bound_statements_equal_brute_force(dims, maxi):
    """The statements the kernels and every host build share (csrc/dsdf_proof.h: block_reduce, block_dilate, window_pass) against numpy
    brute force, exactly, minima and maxima: the blocks of both coarse levels dilated by one block, those of the hit proof by two, and
    the 6^3 window."""
    grid = B.noise(dims)
    for shift, radius in [(s, 1) for s in B.MIN_SHIFTS] + [(B.HIT_SHIFT, B.HIT_RADIUS)]:
        raw, dil = block_bounds(grid, shift, radius, maxi)
        ref_raw, ref_dil = B.block_bounds(grid, shift, radius, maxi)
        assert raw.shape == ref_raw.shape and (raw == ref_raw).all() and (dil == ref_dil).all(), (shift, radius)
    assert (window(grid, maxi) == B.window(grid, maxi)).all()


@pytest.mark.parametrize('name', CASES)
def test_fine_empty_proof_agrees_with_traced_rays(harness, name):
    grid, W, H, origin = case(name)
    cam = O.Camera(origin).params()
    coarse, fine, info = host_flags(harness, name)
    c_emp, c_g = (coarse & PX_EMPTY) != 0, (coarse & PX_EMPTY_G) != 0
    f_emp, f_g = (fine & PX_EMPTY) != 0, (fine & PX_EMPTY_G) != 0
    # the fine set contains the coarse set: the window minima are tighter than the dilated block minima, the step is shorter
    assert (c_emp <= f_emp).all() and (c_g <= f_g).all()
    assert (f_g <= f_emp).all()
    new_p, new_g = f_emp & ~c_emp, f_g & ~c_g
    print(f"{name}: primal-empty {c_emp.sum()} -> {f_emp.sum()} (+{new_p.sum()}), gradient-empty {c_g.sum()} -> {f_g.sum()} (+{new_g.sum()}) "
          f"of {fine.size} film-block pixels")
    # the stage is not vacuous on this case: it settles pixels the block minima leave
    assert new_p.sum() >= 1 and new_g.sum() >= 1
    # every fine-flagged pixel is a miss for every traced sample ray of the primal's march ...
    hits = harness.trace_hits(grid, cam, W, H, spp=SPP, seed=21)
    assert not hits[f_emp].any(), f"{hits[f_emp].any(-1).sum()} pixels flagged empty by the fine stage hold a hitting sample"
    # ... and for bit 1 the differentiable march misses too and the boundary weight of every sample is zero
    sw = sample_weights(harness.params, grid, cam, W, H, SPP, 22, f_g)
    assert not (sw[f_g] & 1).any(), "a pixel flagged gradient-empty holds a hitting sample"
    assert not (sw[f_g] & 2).any(), f"{((sw[f_g] & 2) != 0).any(-1).sum()} pixels flagged gradient-empty hold a sample with a positive boundary weight"
