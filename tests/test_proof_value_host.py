"""CPU check of the THIRD proof stage (csrc/dsdf_proof.h: the spline value on the centre ray -+ a gradient bound, ValueBound /
pixel_fine_proofs) through the stand-alone host build of the fine stages (tests/harness/dsdf_proof_stages_host.cpp), against traced sample rays: every sample
of a pixel the stage newly proves empty must miss, of one it proves gradient-empty must also carry a zero boundary weight, of one it
proves hit must hit.  The render kernels skip the march of such pixels, so a single counter-example would be a wrong image or
gradient: zero violations, no tolerance.  Cases: those of tests/proof_fine_cases.py and one grid of plain random values, no SDF,
whose gradient bound is so large that the stage proves next to nothing.  The merged one-loop form of the second stage must return
exactly the flags of its two-loop form."""
import numpy as np
import pytest

import proof_fine_cases as F
from proof_value_cases import CASES, NOISE, PX_EMPTY, PX_EMPTY_FINE, PX_EMPTY_G, PX_HIT, case, device_camera, host_flags, host_lib, trace

SPP = 16


def test_gradient_bound_is_the_largest_tap_difference():
    grid = case('rag_x3')[0]
    import ctypes as C
    D = np.zeros(3, np.float32)
    rz, ry, rx = grid.shape
    host_lib().psh_tap_diff_max(grid.ctypes.data_as(C.c_void_p), rx, ry, rz, D.ctypes.data_as(C.c_void_p))
    ref = [np.abs(np.diff(grid, axis=ax)).max() for ax in (2, 1, 0)]
    assert D.tolist() == [float(v) for v in ref]


@pytest.mark.parametrize('want_hit', [True, False])
@pytest.mark.parametrize('name', CASES)
def test_merged_loop_returns_the_flags_of_the_two_loops(harness, name, want_hit):
    h = host_flags(harness, name, want_hit)
    assert (h['merged'] == h['two']).all(), f"{int((h['merged'] != h['two']).sum())} pixels differ"
    # the third stage proves whatever the second proves (empty bits; a pixel the second proves hit is proven hit)
    assert ((h['third'] & h['two']) == h['two']).all()


@pytest.mark.parametrize('name', CASES)
def test_third_stage_agrees_with_traced_rays(harness, name):
    h = host_flags(harness, name, True)
    two, third = h['two'], h['third']
    new = third & ~two
    new_p, new_g, new_h = (new & PX_EMPTY_FINE) != 0, (new & PX_EMPTY_G) != 0, (new & PX_HIT) != 0
    print(f"{name}: step {h['info'][0]:.5f}, r {h['info'][1]:.3f} voxels, D {h['info'][2:]}; newly proven: primal-empty {new_p.sum()}, "
          f"gradient-empty {new_g.sum()}, hit {new_h.sum()} of {two.size} film-block pixels "
          f"(second stage: {((two & PX_EMPTY_FINE) != 0).sum()} / {((two & PX_EMPTY_G) != 0).sum()} / {((two & PX_HIT) != 0).sum()})")
    assert not (new_h & (new_p | new_g)).any()
    if name == NOISE:
        # the bound of a grid that is no SDF is large: next to nothing is proven beyond the second stage
        assert new_p.sum() + new_g.sum() + new_h.sum() <= 0.001 * two.size
    else:
        assert new_p.sum() >= 1 and new_g.sum() >= 1 and new_h.sum() >= 1         # the stage is not vacuous on this case
    mask = new_p | new_g | new_h
    if not mask.any():
        return
    t = trace(harness.params, name, SPP, 31, mask)
    assert not (t[new_p] & 1).any(), f"{(t[new_p] & 1).any(-1).sum()} pixels newly proven empty hold a hitting sample"
    assert not (t[new_g] & 2).any(), "a pixel newly proven gradient-empty holds a hitting sample"
    assert not (t[new_g] & 4).any(), f"{((t[new_g] & 4) != 0).any(-1).sum()} pixels newly proven gradient-empty hold a sample with a positive boundary weight"
    assert (t[new_h] & 1).all(), f"{(~((t[new_h] & 1) != 0)).any(-1).sum()} pixels newly proven hit hold a sample that misses"


@pytest.mark.parametrize('name', F.CASES)
def test_host_build_with_the_device_camera_stays_inside_the_allowance(harness, name):
    """tests/test_gpu_proof_value.py compares the device's effective plane with this host build run on the ORACLE's camera record and
    allows mismatches on 0.2 % of the coarse-proven pixels for centre-ray rounding.  The device receives dsdf.Sensor's record instead:
    the host build run with THAT record must stay inside the same allowance on the chosen cases, bit by bit, or the allowance would
    be spent before the device has rounded anything."""
    a = host_flags(harness, name, True)
    cam = device_camera(name)
    b = host_flags(harness, name, True, cam=cam)
    base = int(((a['coarse'] & PX_EMPTY) != 0).sum())
    ref = np.ascontiguousarray(__import__('sdf_oracle').Camera(case(name)[3]).params(), np.float32)
    bad = {bit: int((((a['third'] ^ b['third']) & np.uint8(bit)) != 0).sum()) for bit in (PX_EMPTY_G, PX_HIT, PX_EMPTY_FINE)}
    bad['coarse'] = int(((a['coarse'] ^ b['coarse']) & np.uint8(PX_EMPTY | PX_HIT) != 0).sum())
    print(f"{name}: camera records differ in {int((ref != cam).sum())} of 16 floats (largest {float(np.abs(ref - cam).max()):.2e}); "
          f"mismatches of the host build between them {bad}; allowance {0.002 * base:.1f}")
    assert all(n <= 0.002 * base for n in bad.values()), (bad, base)
