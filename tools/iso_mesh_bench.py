#!/usr/bin/env python3
"""Times the surface extraction (csrc/dsdf_iso.h) on the GPU: `python tools/iso_mesh_bench.py [--out FILE.json]`.

  - the four launches dsdf_iso_sample / _mark / _emit / _refine (24 steps, with normals) one by one, and dsdf.extract_mesh as a whole
    (the launches, the two torch.cumsum scans, the read-back of the two totals, the allocations), at the grid's own resolution for the
    128^3 bench grid (bench.synth_grid(128)) and for 256^3;
  - the sizes of the result, and whether the mesh is closed.
Every time is a host clock around work that ends in a device synchronise, the median (and minimum) of `--reps` runs after a warm-up.
No gate: there is no earlier extraction to compare against.  profiles/iso_mesh.md holds the results."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'differentiable-sdf-rendering_amd', 'python')):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn, reps):
    import torch
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--res', type=int, nargs='*', default=[128, 256])
    a = ap.parse_args()
    import torch
    import dsdf
    from bench import synth_grid
    from dsdf import _lib
    from dsdf.renderer import _ptr, _stream
    assert torch.cuda.is_available(), "needs a GPU"
    lib = dsdf.load()
    res = dict(reps=a.reps, grids={})
    for r in a.res:
        grid = dsdf.SdfGrid(synth_grid(r, 'cuda'))
        n = (r, r, r)
        N = (r + 1) ** 3
        iso = C.c_float(0.0)
        values = torch.empty(N, device='cuda')
        cross = torch.empty(N, dtype=torch.uint8, device='cuda')
        counts = torch.empty(2, N, dtype=torch.int32, device='cuda')
        sample = lambda: _lib.check(lib.dsdf_iso_sample(_ptr(grid.padded), r, r, r, *n, _ptr(values), _stream()))
        mark = lambda: _lib.check(lib.dsdf_iso_mark(_ptr(values), *n, iso, _ptr(cross), _ptr(counts[0]), _ptr(counts[1]), _stream()))
        out = dict(nodes=N)
        out['sample_ms'] = timed(sample, a.reps)
        out['mark_ms'] = timed(mark, a.reps)
        scan = lambda: torch.stack([torch.cumsum(counts[0], 0, dtype=torch.int32), torch.cumsum(counts[1], 0, dtype=torch.int32)])
        ends = scan()
        out['scan_ms'] = timed(scan, a.reps)
        V, F = (int(v) for v in ends[:, -1].tolist())
        offs = (ends - counts).contiguous()
        ve = torch.empty(V, dtype=torch.int32, device='cuda'); faces = torch.empty(F, 3, dtype=torch.int32, device='cuda')
        pos = torch.empty(V, 3, device='cuda'); nrm = torch.empty(V, 3, device='cuda')
        emit = lambda: _lib.check(lib.dsdf_iso_emit(_ptr(values), *n, iso, _ptr(cross), _ptr(offs[0]), _ptr(offs[1]), _ptr(ve), _ptr(faces), _stream()))
        refine = lambda: _lib.check(lib.dsdf_iso_refine(_ptr(grid.padded), r, r, r, _ptr(values), *n, iso, _ptr(ve), V, 24, _ptr(pos), _ptr(nrm),
                                                        _stream()))
        out['emit_ms'] = timed(emit, a.reps)
        out['refine_ms'] = timed(refine, a.reps)
        out['extract_mesh_ms'] = timed(lambda: dsdf.extract_mesh(grid), a.reps)
        v, f, _ = dsdf.extract_mesh(grid)
        assert v.shape[0] == V and f.shape[0] == F
        # closed: every directed edge once, its reverse once
        fl = f.long()
        de = torch.cat([fl[:, [0, 1]], fl[:, [1, 2]], fl[:, [2, 0]]])
        key = de[:, 0] * (V + 1) + de[:, 1]
        rkey = de[:, 1] * (V + 1) + de[:, 0]
        uniq, cnt = torch.unique(key, return_counts=True)
        out.update(vertices=V, faces=F, closed=bool((cnt == 1).all() and torch.isin(rkey, uniq).all()))
        res['grids'][r] = out
        print(json.dumps({r: out}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
