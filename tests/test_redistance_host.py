"""The fp32 arithmetic of the redistancing kernel (csrc/dsdf_eikonal.h) on the CPU against the fp64 oracle.

hh_redistance (tests/harness) runs the KERNEL's initialisation and update functions under the oracle's sequential fast sweep.  The
monotone scheme has one fixed point, so what is left between the two results is the rounding of the fp32 update -- at grids where
the distances are many voxels long and an update that works on the absolute neighbour values loses the discriminant (of order h^2)
in a difference of numbers of order u^2.  Measured errors: profiles/redistance_precision.md."""
import ctypes as C

import numpy as np
import pytest

import redistance_cases as RC

CASES = [('corner', (88, 88, 88)), ('corner', (168, 168, 168)), ('corner', (9, 200, 64)), ('circle', (2, 728, 728)),
         ('centred', (128, 128, 128))]


def hh_redistance(harness, phi, max_rounds=512):
    phi = np.ascontiguousarray(phi, np.float32)
    out = np.zeros_like(phi)
    rz, ry, rx = phi.shape
    rounds = harness.lib.hh_redistance(harness._p(phi), rx, ry, rz, harness._p(out), C.c_int(max_rounds))
    return out, rounds


@pytest.mark.parametrize('kind,shape', CASES, ids=[f"{k}-{'x'.join(map(str, s))}" for k, s in CASES])
def test_kernel_update_matches_fp64_oracle(harness, kind, shape):
    phi, ref = RC.case(kind, shape)
    out, rounds = hh_redistance(harness, phi)
    assert rounds > 0, "the sweeps did not reach their fixed point"
    hmin = min(RC.spacings(shape))
    bound = RC.host_bound(ref)
    err = np.abs(out.astype(np.float64) - ref)
    fz = RC.frozen_mask(phi)
    print(f"redistance host {kind} {shape}: max err {err.max() / hmin:.5f} voxel (bound {bound / hmin:.5f}), frozen {err[fz].max() / hmin:.2e} voxel, "
          f"max |ref| {np.abs(ref).max():.3f}, {rounds} rounds of 8 sweeps")
    assert np.isfinite(out).all() and RC.finite(ref).all()
    assert ((out < 0) == (phi < 0)).all() and ((out < 0) == (ref < 0)).all()         # signs: everywhere, no exclusions
    assert (err[fz] <= 4 * np.spacing(np.abs(ref[fz]).astype(np.float32))).all()     # the frozen band: 4 ulp
    assert err.max() < bound
