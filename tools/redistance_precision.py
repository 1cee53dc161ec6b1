"""Per case of tests/redistance_cases.py: error of dsdf.redistance against the fp64 C oracle, fp64 Godunov residual, work counters
and time -- the GPU lines of profiles/redistance_precision.md (the host lines are printed by tests/test_redistance_host.py -s).

    python tools/redistance_precision.py [--before PATH/libdsdf.so]

--before: a second build of the library (another commit's sources) measured on the same inputs, for a before / after table."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'differentiable-sdf-rendering_amd', 'python')]
import numpy as np
import torch

import redistance_cases as RC
import dsdf
from dsdf import _lib

CASES = [('corner', (88, 88, 88), 1), ('corner', (88, 88, 88), -1), ('corner', (168, 168, 168), 1), ('circle', (2, 728, 728), 1),
         ('corner', (9, 200, 64), 1), ('centred', (128, 128, 128), 1), ('slab', (88, 88, 88), 1), ('slab', (13, 50, 91), 1),
         ('centred', (256, 256, 256), 1), ('corner', (256, 256, 256), 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--before', default=None)
    args = ap.parse_args()
    libs = [('after', _lib.LIB_PATH)] + ([('before', args.before)] if args.before else [])
    handles = {tag: _lib._open(path) for tag, path in libs}
    for kind, shape, sign in CASES:
        t = time.time(); phi, ref = RC.case(kind, shape, sign); t_or = time.time() - t
        hmin = min(RC.spacings(shape))
        for tag, _ in libs:
            _lib._lib = handles[tag]
            p = torch.tensor(phi, device='cuda')
            out, cnt = dsdf.redistance(p, return_counters=True)
            torch.cuda.synchronize()
            ts = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); dsdf.redistance(p); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
            o = out.cpu().numpy(); r, v, ps, st = (int(x) for x in cnt.cpu())
            err = np.abs(o.astype(np.float64) - ref).max() / hmin
            res = RC.godunov_residual(o, phi) / hmin if max(shape) <= 168 else float('nan')
            print(f"{tag:6s} {kind:8s} {str(shape):16s} sign {sign:+d}: err {err:.5f} voxel (gpu bound {RC.gpu_bound(ref) / hmin:.5f}), residual {res:.5f}, "
                  f"tiles {RC.ntiles(shape)}, rounds {r}, visits {v}, passes {ps}, status {st}, signs ok {bool(((o < 0) == (phi < 0)).all())}, "
                  f"median {np.median(ts):.3f} ms, oracle {t_or:.1f} s", flush=True)


if __name__ == '__main__':
    main()
