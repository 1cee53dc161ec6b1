#!/usr/bin/env python3
"""Times and measures the mesh simplification (csrc/dsdf_simplify.h) on the GPU: `python tools/mesh_simplify_bench.py [--md FILE] [--out FILE.json]`.

  - timing: dsdf.simplify_mesh (normals on) at 32 and 64 cells on the mesh dsdf.extract_mesh gives on the 128^3 bench grid
    (tests/golden/bench_grid128.npz), next to that extract_mesh call, and the same sequence through the C ABI stage by stage: the three
    entry points against the torch sort / unique / scans between them;
  - errors: max |x_fp32 - x_fp64| / cell size against the fp64 reference (tests/mesh_simplify_oracle.py) on the case table of the tests,
    for the device and for the host build of the same statements (tests/harness/dsdf_simplify_host.cpp), and whether the two agree bit
    for bit.
Every time is a host clock around work that ends in a device synchronise, the median (and minimum) of `--reps` runs after a warm-up; the
stages are synchronised one by one, so their sum exceeds the whole call.  It writes the tables to profiles/mesh_simplify.md (--md);
nothing gates a time."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'differentiable-sdf-rendering_amd', 'python')):
    if p not in sys.path:
        sys.path.insert(0, p)

STAGES = ('keys kernel', 'sort + unique + starts (torch)', 'mark kernel', 'scans + totals (torch)', 'emit kernels')


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


def staged(dsdf, vert, fac, cells, lo, hi, reps):
    """The sequence of dsdf.simplify_mesh through the C ABI with a synchronise after every stage -> {stage: (median ms, min ms)}."""
    import torch
    lib = dsdf.load()
    dev = vert.device
    F = int(fac.shape[0])
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    lo_c, hi_c = (C.c_float * 3)(*lo), (C.c_float * 3)(*hi)
    i32 = lambda *s, z=False: (torch.zeros if z else torch.empty)(*s, dtype=torch.int32, device=dev)
    laps = {s: [] for s in STAGES}
    for rep in range(reps + 1):
        marks = []

        def lap():
            torch.cuda.synchronize()
            marks.append(time.perf_counter())
        lap()
        keys = i32(3 * F)
        assert lib.dsdf_simplify_keys(ptr(vert), ptr(fac), F, lo_c, hi_c, *cells, ptr(keys), None) == 0
        lap()
        sorted_keys, order = torch.sort(keys, stable=True)
        corner = order.to(torch.int32)
        cell_keys, counts = torch.unique_consecutive(sorted_keys, return_counts=True)
        U = int(cell_keys.shape[0])
        start = i32(U + 1, z=True)
        start[1:] = torch.cumsum(counts, 0)
        lap()
        rank, keep, used = i32(3 * F), i32(F), i32(U, z=True)
        assert lib.dsdf_simplify_mark(ptr(keys), F, ptr(cell_keys), U, ptr(rank), ptr(keep), ptr(used), None) == 0
        lap()
        v_end, f_end = torch.cumsum(used, 0, dtype=torch.int32), torch.cumsum(keep, 0, dtype=torch.int32)
        Vn, Fn = (int(t) for t in torch.stack([v_end[-1], f_end[-1]]).tolist())
        vid, foff = v_end - used, f_end - keep
        lap()
        fo, pos, nrm = i32(Fn, 3), torch.empty(Vn, 3, device=dev), torch.empty(Vn, 3, device=dev)
        assert lib.dsdf_simplify_emit(ptr(vert), ptr(fac), F, None, lo_c, hi_c, *cells, C.c_float(1e-3), ptr(corner), ptr(cell_keys), ptr(start), U,
                                      ptr(rank), ptr(keep), ptr(foff), ptr(used), ptr(vid), ptr(fo), ptr(pos), ptr(nrm), None, None) == 0
        lap()
        if rep:                                                    # (the first pass warms up)
            for s, a, b in zip(STAGES, marks, marks[1:]):
                laps[s].append((b - a) * 1e3)
    return {s: (statistics.median(t), min(t)) for s, t in laps.items()}, (Vn, Fn, U)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=os.path.join(ROOT, 'profiles', 'mesh_simplify.md'))
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=7)
    a = ap.parse_args()
    import numpy as np
    import torch
    import dsdf
    import mesh_simplify_oracle as O
    import test_mesh_simplify_host as H
    assert torch.cuda.is_available(), "needs a GPU"
    dsdf.load()
    res = dict(reps=a.reps, device=torch.cuda.get_device_name(0), timing={}, errors={})
    grid = dsdf.SdfGrid(torch.from_numpy(np.load(os.path.join(ROOT, 'tests', 'golden', 'bench_grid128.npz'))['grid']).float().cuda())
    v, f, n = dsdf.extract_mesh(grid)
    res['extract'] = dict(vertices=int(v.shape[0]), faces=int(f.shape[0]), ms=timed(lambda: dsdf.extract_mesh(grid), a.reps))
    print(json.dumps(res['extract']), flush=True)
    lo_t, hi_t = v.amin(0).double(), v.amax(0).double()
    g = dsdf.renderer.SIMPLIFY_GROW * float((hi_t - lo_t).max())
    lo, hi = (lo_t - g).float().tolist(), (hi_t + g).float().tolist()
    for cells in (32, 64):
        c3 = dsdf.renderer.resolve_cells(cells, lo, hi)
        out = dsdf.simplify_mesh(v, f, cells, normals=True)
        stages, (Vn, Fn, U) = staged(dsdf, v, f, c3, lo, hi, a.reps)
        assert (Vn, Fn) == (int(out[0].shape[0]), int(out[1].shape[0]))
        D = O.diagonal(lo, hi, c3)
        d = dsdf.mesh_distance(out[0][out[1].long()], v[f.long()], n=200_000)
        r = dict(cells=list(c3), vertices=Vn, faces=Fn, occupied=U, ms=timed(lambda: dsdf.simplify_mesh(v, f, cells, normals=True), a.reps),
                 stages=stages, out_to_in_max_D=d['a_to_b_max'] / D, in_to_out_max_D=d['b_to_a_max'] / D)
        res['timing'][cells] = r
        print(json.dumps({cells: r}), flush=True)
    host = H.load_host()
    for name, (mname, box, cells) in O.CASES.items():
        vv, ff = O.mesh(mname)
        col = O.colors_of(vv)
        ref = O.reference(name)
        hst = H.simplify(host, vv, ff, box[0], box[1], cells, colors=col)
        dev = dsdf.simplify_mesh(torch.from_numpy(vv).cuda(), torch.from_numpy(ff.astype(np.int32)).cuda(), cells, bounds=box, normals=True,
                                 colors=torch.from_numpy(col).cuda())
        dv = dict(vertices=dev[0].cpu().numpy(), faces=dev[1].cpu().numpy(), normals=dev[2].cpu().numpy(), colors=dev[3].cpu().numpy())
        same = all(dv[k].shape == hst[k].shape and np.array_equal(dv[k].view(np.int32), hst[k].view(np.int32)) for k in dv)
        e = dict(faces_in=int(len(ff)), faces_out=int(len(ref['faces'])), vertices_out=int(len(ref['vertices'])), clamped=int(ref['clamped'].sum()),
                 host=H.position_error(hst, ref, box, cells), device=H.position_error(dv, ref, box, cells), same_bits=bool(same))
        res['errors'][name] = e
        print(json.dumps({name: e}), flush=True)
    ms = lambda t: f'{t[0]:.3f} ({t[1]:.3f})'
    ex = res['extract']
    lines = ['# Mesh simplification (vertex clustering with quadric errors): timings and errors', '',
             f"`python tools/mesh_simplify_bench.py` on {res['device']}: host clock around work that ends in a device synchronise, median (minimum) of "
             f"{a.reps} runs after a warm-up.", '',
             f"## `dsdf.simplify_mesh` (normals on) on the mesh of the 128^3 bench grid: {ex['vertices']} vertices, {ex['faces']} faces", '',
             f"The `dsdf.extract_mesh` call that produced it: {ms(ex['ms'])} ms.  Distances: the sampled maxima of `dsdf.mesh_distance` "
             "(200 k points each way) in cell diagonals D.", '',
             '| cells | grid | occupied cells | vertices out | faces out | simplify_mesh ms | out -> in max / D | in -> out max / D |', '|---|---|---|---|---|---|---|---|']
    for cells, r in res['timing'].items():
        lines.append(f"| {cells} | {' x '.join(str(c) for c in r['cells'])} | {r['occupied']} | {r['vertices']} | {r['faces']} | {ms(r['ms'])} | "
                     f"{r['out_to_in_max_D']:.3f} | {r['in_to_out_max_D']:.3f} |")
    lines += ['', '## The same sequence through the C ABI, synchronised after every stage (so the sum exceeds the whole call)', '',
              '| cells | ' + ' | '.join(f'{s} ms' for s in STAGES) + ' |', '|---|' + '---|' * len(STAGES)]
    for cells, r in res['timing'].items():
        lines.append(f'| {cells} | ' + ' | '.join(ms(r['stages'][s]) for s in STAGES) + ' |')
    lines += ['', '## Errors against the fp64 reference (tests/mesh_simplify_oracle.py), the case table of the tests', '',
              'max |x_fp32 - x_fp64| / cell size over the output vertices and axes.  Host: the g++ build of the same statements (its largest '
              'error is `MEASURED_MAX_ERR`); same bits: faces, positions, normals and colours of the device `==` the host build.', '',
              '| case | faces in | faces out | vertices out | clamped | host | device | same bits |', '|---|---|---|---|---|---|---|---|']
    for name, e in res['errors'].items():
        lines.append(f"| {name} | {e['faces_in']} | {e['faces_out']} | {e['vertices_out']} | {e['clamped']} | {e['host']:.3e} | {e['device']:.3e} | "
                     f"{'yes' if e['same_bits'] else 'NO'} |")
    lines.append('')
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, 'w') as fh:
        fh.write('\n'.join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
