#!/usr/bin/env python3
"""Times the connected components of a mesh (csrc/dsdf_components.h) on the GPU: `python tools/mesh_components_bench.py [--md FILE] [--out FILE.json]`.

  - inputs: the mesh dsdf.extract_mesh gives on the 128^3 bench grid (tests/golden/bench_grid128.npz), and a synthetic mesh of many small
    parts: `--parts` icospheres of 80 faces each with their vertex numbers shuffled over the whole mesh;
  - the labelling call (dsdf_mesh_components: three launches) between two device events, and the whole dsdf.mesh_components call with
    vertices (labels, numbering, areas, volumes, boxes, boundary edges) by a host clock around work that ends in a device synchronise:
    median (minimum) of `--reps` runs after a warm-up;
  - beside them on the same input, on the CPU: the union-find of tests/mesh_components_oracle.py (plain Python, one run) and, where scipy
    imports, scipy.sparse.csgraph.connected_components on the vertex graph (median of three); every result is compared with the device's.
It writes the tables to profiles/mesh_components.md (--md); nothing gates a time."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'differentiable-sdf-rendering_amd', 'python')):
    if p not in sys.path:
        sys.path.insert(0, p)


def host_timed(fn, reps):
    import torch
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def event_timed(fn, reps):
    import torch
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def many_parts(n, seed=0):
    """n icospheres of 80 faces on a lattice, the vertex numbers of the whole mesh shuffled."""
    import numpy as np
    import mesh_oracle as M
    v0, f0 = M.icosphere(0.3, 1)
    side = int(np.ceil(n ** (1 / 3)))
    k = np.arange(n)
    centres = np.stack([k % side, (k // side) % side, k // (side * side)], -1).astype(np.float32)
    v = (v0[None] + centres[:, None]).reshape(-1, 3)
    f = (f0[None] + (k * len(v0))[:, None, None]).reshape(-1, 3)
    new = np.random.default_rng(seed).permutation(len(v))
    vv = np.empty_like(v)
    vv[new] = v
    return vv, new[f]


def measure(dsdf, name, vert, fac, reps):
    import numpy as np
    import torch
    import mesh_components_oracle as O
    lib = dsdf.load()
    V, F = int(vert.shape[0]), int(fac.shape[0])
    label = torch.empty(V, dtype=torch.int32, device='cuda')
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def labelling():
        assert lib.dsdf_mesh_components(ptr(fac), F, V, ptr(label), ptr(status), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    r = dict(vertices=V, faces=F, labelling_ms=event_timed(labelling, reps))
    assert int(status.item()) == 0
    comp = dsdf.mesh_components(fac, vertices=vert)
    r['components'] = comp.n
    r['closed'] = int((comp.boundary_edges == 0).sum())
    r['full_ms'] = host_timed(lambda: dsdf.mesh_components(fac, vertices=vert), reps)
    r['labels_only_ms'] = host_timed(lambda: dsdf.mesh_components(fac, n_vertices=V), reps)
    f = fac.cpu().numpy().astype(np.int64)
    dev_label = label.cpu().numpy()
    t0 = time.perf_counter()
    ref = O.labels(f, V)
    r['cpu_union_find_ms'] = (time.perf_counter() - t0) * 1e3
    r['same_as_cpu_union_find'] = bool(np.array_equal(ref, dev_label))
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import connected_components
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            i, j = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
            n, theirs = connected_components(sp.coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(V, V)), directed=False)
            ts.append((time.perf_counter() - t0) * 1e3)
        first = np.full(n, V)
        np.minimum.at(first, theirs, np.arange(V))
        r['scipy_ms'] = statistics.median(ts)
        r['same_as_scipy'] = bool(np.array_equal(first[theirs], dev_label))
    except ImportError:
        r['scipy_ms'] = None
    print(json.dumps({name: r}), flush=True)
    return r


def commit():
    try:
        return subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip() or None
    except OSError:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=os.path.join(ROOT, 'profiles', 'mesh_components.md'))
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--parts', type=int, default=20000)
    ap.add_argument('--commit', default=None, help='what the working tree is (default: git rev-parse HEAD, where this is a git checkout)')
    a = ap.parse_args()
    import numpy as np
    import torch
    import dsdf
    assert torch.cuda.is_available(), "needs a GPU"
    dsdf.load()
    res = dict(reps=a.reps, device=torch.cuda.get_device_name(0), commit=a.commit or commit() or 'not recorded', inputs={})
    grid = dsdf.SdfGrid(torch.from_numpy(np.load(os.path.join(ROOT, 'tests', 'golden', 'bench_grid128.npz'))['grid']).float().cuda())
    v, f, _ = dsdf.extract_mesh(grid)
    res['inputs']['extract_mesh of the 128^3 bench grid'] = measure(dsdf, 'bench grid', v, f, a.reps)
    pv, pf = many_parts(a.parts)
    res['inputs'][f'{a.parts} icospheres of 80 faces, vertex numbers shuffled'] = measure(
        dsdf, 'many parts', torch.from_numpy(pv).cuda(), torch.from_numpy(pf.astype(np.int32)).cuda(), a.reps)
    ms = lambda t: f'{t[0]:.3f} ({t[1]:.3f})'
    lines = ['# Connected components of a mesh (lock-free union-find over the index buffer): timings', '',
             f"`python tools/mesh_components_bench.py` on {res['device']}, working tree: {res['commit']}.  Median (minimum) of {a.reps} runs after a "
             "warm-up.  Labelling: `dsdf_mesh_components` (three launches) between two device events.  `mesh_components`: the whole call by a "
             "host clock around work that ends in a device synchronise -- with vertices (labels, numbering, areas, volumes, boxes, boundary "
             "edges) and with the vertex count alone (labels and numbering).  CPU: the plain-Python union-find of "
             "tests/mesh_components_oracle.py (one run) and scipy.sparse.csgraph.connected_components on the vertex graph, building the "
             "sparse matrix included (median of three), on the same index buffer; `same` = their labels `==` the device's.  No path shortening "
             "is implemented, so there is no A/B of it.", '',
             '| input | vertices | faces | components (closed) | labelling ms | mesh_components ms | labels and numbering only ms | CPU union-find ms | scipy ms | same |',
             '|---|---|---|---|---|---|---|---|---|---|']
    for name, r in res['inputs'].items():
        same = r['same_as_cpu_union_find'] and r.get('same_as_scipy', True)
        lines.append(f"| {name} | {r['vertices']} | {r['faces']} | {r['components']} ({r['closed']}) | {ms(r['labelling_ms'])} | {ms(r['full_ms'])} | "
                     f"{ms(r['labels_only_ms'])} | {r['cpu_union_find_ms']:.0f} | {'not installed' if r['scipy_ms'] is None else format(r['scipy_ms'], '.1f')} | "
                     f"{'yes' if same else 'NO'} |")
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
