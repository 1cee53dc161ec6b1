#!/usr/bin/env python3
"""Offline replay (CPU, test infrastructure: uses oracle/ and tests/harness), sibling of tools/sim_gradient_bound.py: how much of
k_pixel_hit_fine's loop does the interval [ta, tb] of csrc/dsdf_proof.h (proof_interval: two walks through the dilated 8^3 minima)
remove on the bench views?  Runs the HOST BUILD of both forms of the fine stages (tests/harness/dsdf_proof_interval_host.cpp) on the
pixels k_pixel_skip lists and reports, per view:

  * loop rounds per pixel, before and after (full rounds; after: also the light rounds of the prefix, which load the window maxima for
    the hit proof's landing bound, and the leaps, which only advance t);
  * loop rounds per WAVE: 64 consecutive list entries (row-major: the order inside one wave of k_pixel_skip's compaction), the maximum
    over the lanes of each kind of round -- a wave runs each loop as long as its slowest lane;
  * fetches of the window minima, the window maxima and spline values, and the loads of the walks.

    python tools/sim_proof_interval.py [views, comma-separated: default 0,4,8]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'differentiable-sdf-rendering_amd', 'python')):
    sys.path.insert(0, p)
import sdf_oracle as O
import __graft_entry__ as g
import proof_interval_cases as I
from bench import synth_grid
from conftest import HostHarness

PX_EMPTY, PX_EMPTY_G, PX_HIT = 1, 2, 16


def main():
    views = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else '0,4,8').split(',')]
    res, W = 256, 512
    grid = np.ascontiguousarray(synth_grid(res, 'cpu').numpy(), np.float32)
    hh = HostHarness(g.build_harness())
    for view in views:
        t0 = time.time()
        cam = np.ascontiguousarray(O.Camera(O.regular_camera_origins(12)[view]).rounded().params(), np.float32)
        coarse, _ = hh.pixel_proof(grid, cam, W, W, stages=1)
        # what k_pixel_skip lists when a gradient pass reads the flags (list_g), and which of those want the hit proof
        listed = ((coarse & (PX_EMPTY | PX_HIT)) == 0) | ((coarse & 3) == PX_EMPTY)
        want_hit = (coarse & PX_EMPTY) == 0
        r = I.proofs(hh.params, grid, cam, W, W, want_hit, True, listed)
        assert (r['ref'] == r['near'])[listed].all()
        cnt = r['cnt'][listed].astype(np.int64)                      # (n, form, counter), row-major list order
        n = cnt.shape[0]
        low = r['near'][listed] & 0xff
        third = r['near'][listed] >> 8
        ta, tb, t0r, t1r = (r['ival'][listed][:, k] for k in range(4))
        print(f'==== view {view}: {n} listed pixels ({want_hit[listed].sum()} with the hit proof); second stage proves empty '
              f'{((low & 3) != 0).sum()}, hit {((low & PX_HIT) != 0).sum()}; third stage empty {((third & 3) != 0).sum()}, hit '
              f'{((third & PX_HIT) != 0).sum()}, neither {(third == 0).sum()}; empty interval {(ta > tb).sum()}; mean share of the ray '
              f'inside [ta, tb] {np.mean(np.where(ta > tb, 0, (tb - ta) / np.maximum(t1r - t0r, 1e-9))):.3f}   [{time.time() - t0:.0f}s]')
        names = I.COUNTERS
        tot = cnt.sum(0)
        for f, form in enumerate(('before', 'after ')):
            print(f'  {form} per pixel: ' + ', '.join(f'{k} {tot[f][i] / n:.1f}' for i, k in enumerate(names)))
        pad = (-n) % 64
        w = np.concatenate([cnt, np.zeros((pad,) + cnt.shape[1:], np.int64)]).reshape(-1, 64, 2, len(names)).max(1)      # (waves, form, counter)
        ws = w.sum(0)
        kinds = [names.index(k) for k in ('round', 'light', 'leap')]
        print(f'  per wave ({w.shape[0]} waves), maximum over the lanes: before round {ws[0][0] / w.shape[0]:.1f}; after ' +
              ', '.join(f'{names[i]} {ws[1][i] / w.shape[0]:.1f}' for i in kinds) +
              f', walk rounds of four loads {np.ceil(w[:, 1, names.index("walk")] / 8).sum() / w.shape[0]:.1f} (x2 walks)')
        print(f'  wave rounds after / before: full rounds alone {ws[1][0] / ws[0][0]:.3f}; with a light round counted as half a full one '
              f'{(ws[1][0] + 0.5 * ws[1][1]) / ws[0][0]:.3f}; lane rounds {tot[1][0] / tot[0][0]:.3f}', flush=True)


if __name__ == '__main__':
    main()
