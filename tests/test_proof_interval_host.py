"""CPU check of the restricted loop of the fine proof stages (csrc/dsdf_proof.h: proof_interval, pixel_fine_proofs_near -- what
k_pixel_hit_fine runs) through the stand-alone host build tests/harness/dsdf_proof_interval_host.cpp: the form that walks only the
stretch [ta, tb] of the centre ray near the shape must return, for EVERY film-block pixel, the two bytes (second stage, third stage) of
the reference form that walks the ray from box entry to box exit -- no tolerance; and the certificate behind it is checked position
by position against window minima computed from their definition."""
import numpy as np
import pytest

import proof_interval_cases as I
from proof_value_cases import CASES, case

PX_HIT = 16
# grids of proof_interval_cases: film size, field of view -- the fine stages need a sample ray within 0.01 of the SHORTEST axis of its
# centre ray (ProofMargins: the box argument), so the noise grid, 16 voxels thin, gets a narrow view of its middle
OWN = {'halfspace64': (176, 39.0), 'slab64': (176, 39.0), 'plate64': (176, 39.0), 'noise_rag': (160, 16.0)}


def _scene(name):
    if name in OWN:
        return I.grid(name), OWN[name][0], OWN[name][0], I.camera(2, fov=OWN[name][1])
    g, W, H, origin = case(name)
    import sdf_oracle as O
    return g, W, H, np.ascontiguousarray(O.Camera(origin).params(), np.float32)


_res = {}


def _proofs(harness, name, want_hit, third=True):
    """computed once per case, shared, never modified"""
    key = (name, want_hit, third)
    if key not in _res:
        g, W, H, cam = _scene(name)
        r = I.proofs(harness.params, g, cam, W, H, want_hit, third)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _res[key] = r
    return _res[key]


def _describe(name, r):
    ta, tb, t0, t1 = (r['ival'][..., k] for k in range(4))
    met = np.isfinite(t1) & (t1 > 0) & (t1 >= t0)
    c = r['cnt'].astype(np.int64).sum((0, 1))
    print(f"{name}: cstep {r['cstep']:.4f}; pixels {met.sum()}: empty interval {(met & (ta > tb)).sum()}, ta == t0 {(met & (ta == t0)).sum()}, "
          f"tb == t1 {(met & (tb == t1)).sum()}, ray shorter than a coarse step {(met & (t1 - t0 < r['cstep'])).sum()}; "
          f"reference {dict(zip(I.COUNTERS, c[0].tolist()))} restricted {dict(zip(I.COUNTERS, c[1].tolist()))}")
    return met, ta, tb, t0, t1


@pytest.mark.parametrize('want_hit', [True, False])
@pytest.mark.parametrize('name', CASES + sorted(OWN))
def test_restricted_form_returns_the_reference_flags(harness, name, want_hit):
    r = _proofs(harness, name, want_hit)
    _describe(name, r)
    bad = r['ref'] != r['near']
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} pixels differ, first {np.argwhere(bad)[:4].tolist()}: " \
                          f"{r['ref'][bad][:4].tolist()} vs {r['near'][bad][:4].tolist()}"
    # not vacuous: the restricted form runs fewer full rounds, and both bytes carry proofs
    c = r['cnt'].astype(np.int64).sum((0, 1))
    if name == 'noise64':         # (values below 0 in every 8^3 block: the interval is the whole ray, the form must cope)
        assert c[1][0] == c[0][0]
    else:
        assert c[1][0] < c[0][0]
        assert (r['ref'] & 0xff).any() and (r['ref'] >> 8).any()


def test_second_stage_alone(harness):
    """Without the third stage (no gradient bound: the one-plane buffer of a caller) the low byte is all there is."""
    r = _proofs(harness, 'blob64_flat', True, third=False)
    assert (r['ref'] == r['near']).all() and (r['ref'] >> 8 == 0).all() and r['ref'].any()


def test_the_cases_that_can_go_wrong_are_there(harness):
    """The flags above are compared on every pixel; this asserts that those pixels include each kind the restriction could get wrong."""
    met, ta, tb, t0, t1 = _describe('sphere64', _proofs(harness, 'sphere64', True))
    assert (met & (ta > tb)).sum() > 100, "pixels whose interval is empty"
    for name in CASES + sorted(OWN):
        r = _proofs(harness, name, True)
        met, ta, tb, t0, t1 = _describe(name, r)
        if name != 'noise64':      # (values below 0 in every block: the interval is the whole ray)
            assert (met & (ta <= tb) & ((ta > t0) | (tb < t1))).sum() > 100, name
    met, ta, tb, t0, t1 = _describe('rag_x3', _proofs(harness, 'rag_x3', True))
    assert (met & (t1 - t0 < _proofs(harness, 'rag_x3', True)['cstep'])).sum() >= 1, "a ray shorter than one coarse step"
    r = _proofs(harness, 'halfspace64', True)
    met, ta, tb, t0, t1 = _describe('halfspace64', r)
    assert (met & (ta == t0) & (ta <= tb)).sum() > 50, "the surface at the entry face"
    assert (met & (tb == t1) & (ta > t0) & (ta <= tb)).sum() > 50, "the shape reaching the exit"
    short = met & (t1 - t0 < r['cstep'])
    assert short.sum() >= 1
    # two voxels thick: the runs are there (window maxima tightened by the value fall below 0) but none outlasts the landing bound J the
    # prefix feeds -- no hit in either form, after light rounds; six voxels thick: hits proven behind such a prefix
    light = lambda r: r['cnt'][:, :, 1, I.COUNTERS.index('light')] > 0
    r = _proofs(harness, 'slab64', True)
    _describe('slab64', r)
    assert not ((r['near'] | r['near'] >> 8) & PX_HIT).any() and light(r).sum() > 1000
    r = _proofs(harness, 'plate64', True)
    _describe('plate64', r)
    hit3 = ((r['near'] >> 8) & PX_HIT) != 0
    assert (hit3 & light(r)).sum() > 20, int(hit3.sum())


@pytest.mark.parametrize('icam', [0, 2, 3])
def test_certificate_against_brute_force(harness, icam):
    """Every fine position outside [ta, tb] has a fine window minimum above max(thr_hi, 0): the minima from their definition, the
    positions on the loop's own lattice, all film-block pixels of a (17, 16, 33) noise grid."""
    g = I.grid('noise_rag')
    assert g.shape == I.NOISE_SHAPE
    wmin = _wmin()
    W = H = OWN['noise_rag'][0]
    c = I.certificate(harness.params, g, wmin, I.camera(icam, fov=OWN['noise_rag'][1]), W, H)
    ta, tb, t0, t1 = (c['ival'][..., k] for k in range(4))
    has = c['n'] > 0
    print(f"camera {icam}: {has.sum()} of {has.size} pixels hold {int(c['n'].sum())} positions outside their interval; "
          f"empty intervals {(has & (ta > tb)).sum()}, proper ones {(has & (ta <= tb)).sum()}; smallest margin "
          f"{float((c['min'] - c['thr'])[has].min()):.4f}")
    assert (has & (ta <= tb)).sum() > 200
    if icam == 3:
        assert (has & (ta > tb)).sum() > 50
    bad = has & ~(c['min'] > c['thr'])
    assert not bad.any(), f"{int(bad.sum())} pixels: a window minimum at or below the threshold outside [ta, tb], first {np.argwhere(bad)[:4].tolist()}"


_w = []


def _wmin():
    if not _w:
        w = I.window_min_brute(I.grid('noise_rag'))
        w.setflags(write=False)
        _w.append(w)
    return _w[0]
