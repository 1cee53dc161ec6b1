"""`dsdf.redistance` (csrc/dsdf_redistance.h) against the fp64 C oracle where its scheduler and its fp32 arithmetic are strained.

The kernel launches min(ntiles, 8192) single-wave blocks (a multiple of 32) that stride over 32 sub-lists of the active-tile list, and
drops to 1024 blocks after half of its round budget max_iter = 1.25 (ntx + nty + ntz) + 8.  A block takes a SECOND tile -- the LDS
tile is reused -- only when ntiles > 8192 or when work is left after the grid has shrunk; the cases below are the smallest that get
there, next to partial tiles, fewer tiles than sub-lists, and interfaces the sphere tests do not have.

Every case: max |out - ref| over ALL voxels within redistance_cases.gpu_bound (derived there, not tuned), the sign of phi kept
exactly, status == 0, at least one working round and every tile visited.  Measured figures: profiles/redistance_precision.md."""
import numpy as np
import pytest
import torch

import redistance_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    return m


def run_and_check(dsdf, name, phi, ref):
    out, cnt = dsdf.redistance(torch.tensor(phi, device='cuda'), return_counters=True)
    out = out.cpu().numpy()
    rounds, visits, passes, status = (int(v) for v in cnt.cpu())
    shape = phi.shape
    hmin = min(RC.spacings(shape))
    f = RC.finite(ref)
    bound = RC.gpu_bound(ref)
    err = np.abs(out.astype(np.float64) - ref)
    emax = float(err[f].max()) if f.any() else 0.0
    print(f"redistance gpu {name} {shape}: max err {emax / hmin:.5f} voxel (bound {bound / hmin:.5f}), {RC.ntiles(shape)} tiles, "
          f"rounds {rounds}, visits {visits}, passes {passes}, status {status}")
    assert status == 0                                           # the fixed point was reached within the round budget
    assert rounds >= 1 and visits >= RC.ntiles(shape)
    assert out.shape == shape and not np.isnan(out).any()
    assert ((out < 0) == (phi < 0)).all()                        # the sign of phi, exactly, everywhere
    assert np.array_equal(out[~f], ref[~f].astype(np.float32))   # voxels no front reaches: exactly +-1e10, as the oracle
    assert emax < bound
    return out


# 88^3: 1331 tiles, budget 49 rounds; the grid drops to 1024 blocks at round 24 while the front still has a Manhattan tile distance
# of 30 to go, and the sub-lists hold up to 42 entries for a stride of 32.  sign -1: the far field is negative.
@pytest.mark.parametrize('sign', [1, -1])
def test_shrunk_grid_and_strained_budget(dsdf, sign):
    run_and_check(dsdf, f'corner sphere, sign {sign:+d}', *RC.case('corner', (88, 88, 88), sign))


# ntiles > 8192: blocks take a second tile from round 0 on.  168^3: 9261 tiles, isotropic update; 2 x 728 x 728: 8281 tiles,
# hz = 364 hx, anisotropic update.
def test_stride_loop_isotropic_and_fixed_point(dsdf):
    phi, ref = RC.case('corner', (168, 168, 168))
    out = run_and_check(dsdf, 'corner sphere', phi, ref)
    # independent of any sweep order: the result is a fixed point of the fp64 Godunov update to within the same bound (the fp64
    # oracle's own residual is 3e-8 voxel)
    res = RC.godunov_residual(out, phi)
    print(f"redistance gpu corner sphere (168, 168, 168): fp64 Godunov residual {res * 168:.5f} voxel")
    assert res < RC.gpu_bound(ref)


def test_stride_loop_anisotropic(dsdf):
    run_and_check(dsdf, 'corner circle', *RC.case('circle', (2, 728, 728)))


# partial tiles in every axis, fewer tiles than sub-lists, dimensions below one tile, a single voxel
PARTIAL = [('corner', (83, 21, 9)), ('centred', (13, 50, 91)), ('centred', (16, 16, 16)), ('normal', (3, 5, 2)), ('normal', (1, 1, 9)),
           ('normal', (1, 1, 1))]


@pytest.mark.parametrize('kind,shape', PARTIAL, ids=[f"{k}-{'x'.join(map(str, s))}" for k, s in PARTIAL])
def test_partial_tiles_and_few_sublists(dsdf, kind, shape):
    run_and_check(dsdf, kind, *RC.case(kind, shape))


# two spheres and a slab about one voxel thick that runs into the grid boundary: thin negative regions, a large frozen share
@pytest.mark.parametrize('shape', [(88, 88, 88), (13, 50, 91)], ids=['88x88x88', '13x50x91'])
def test_thin_slab_interface(dsdf, shape):
    phi, ref = RC.case('slab', shape)
    print(f"slab {shape}: negative share {np.mean(phi < 0):.3f}, frozen share {np.mean(RC.frozen_mask(phi)):.3f}")
    assert (phi < 0).any() and 0.02 < np.mean(RC.frozen_mask(phi)) < 0.5
    run_and_check(dsdf, 'spheres + slab', phi, ref)


def test_single_exact_zero(dsdf):
    phi, ref = RC.case('zero', (9, 10, 11))
    out = run_and_check(dsdf, 'single zero', phi, ref)
    assert out[4, 5, 6] == 0.0


@pytest.mark.parametrize('sign', [1, -1])
def test_no_interface(dsdf, sign):
    phi, ref = RC.case('ones', (9, 10, 11), sign)
    out = run_and_check(dsdf, f'all {sign:+d}', phi, ref)
    assert (out == np.float32(sign * RC.RD_BIG)).all() and (ref == sign * RC.RD_BIG).all()
