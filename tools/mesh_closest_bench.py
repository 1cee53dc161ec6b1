#!/usr/bin/env python3
"""Times the closest-point queries (csrc/dsdf_bvh.h, csrc/dsdf_mesh.h) on the GPU: `python tools/mesh_closest_bench.py [--md FILE] [--out FILE.json]`.

  - dsdf.MeshBvh.closest against the brute-force dsdf.mesh_closest for 1 M random points in [-0.5, 0.5]^3 and for the voxel centres of a
    128^3 grid, on icospheres of 1.3 k, 5 k, 20 k and 82 k triangles, with the results compared bit for bit;
  - `mesh_to_sdf.refine` at 64^3 (20 k triangles) with distance='closest' against distance='rays', both through the BVH.
Every time is a host clock around work that ends in a device synchronise, the median (and minimum) of `--reps` runs after a warm-up.
It writes the table to profiles/mesh_closest.md (--md); nothing gates a time."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'differentiable-sdf-rendering_amd', 'python')):
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
    ap.add_argument('--md', default=os.path.join(ROOT, 'profiles', 'mesh_closest.md'))
    ap.add_argument('--out', default=None)
    ap.add_argument('--points', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=7)
    a = ap.parse_args()
    import torch
    import dsdf
    import mesh_oracle as M
    import mesh_to_sdf
    import redistancing
    assert torch.cuda.is_available(), "needs a GPU"
    dsdf.load()
    g = torch.Generator(device='cuda').manual_seed(1)
    sets = {'random': (torch.rand(a.points, 3, device='cuda', generator=g) - 0.5).contiguous(), 'voxels128': mesh_to_sdf.voxel_centres(128, 'cuda')}
    res = dict(points=a.points, reps=a.reps, device=torch.cuda.get_device_name(0), meshes={})
    rows = []
    for subdiv in (3, 4, 5, 6):
        v, f = M.icosphere(0.3, subdiv, centre=(0.05, -0.02, 0.01))
        tri = torch.from_numpy(v[f]).cuda()
        T = int(tri.shape[0])
        r = dict(triangles=T, build_ms=timed(lambda: dsdf.MeshBvh(tri), a.reps))
        bvh = dsdf.MeshBvh(tri)
        for name, x in sets.items():
            r[f'{name}_bvh_ms'] = timed(lambda: bvh.closest(x), a.reps)
            r[f'{name}_brute_ms'] = timed(lambda: dsdf.mesh_closest(tri, x), max(3, a.reps // 2))
            d0, p0 = bvh.closest(x, return_prim=True)
            d1, p1 = dsdf.mesh_closest(tri, x, return_prim=True)
            r[f'{name}_bitwise_equal'] = bool(torch.equal(d0.view(torch.int32), d1.view(torch.int32)) and torch.equal(p0, p1))
            rows.append((T, name, int(x.shape[0]), r['build_ms'][0], r[f'{name}_bvh_ms'], r[f'{name}_brute_ms'], r[f'{name}_bitwise_equal']))
        res['meshes'][T] = r
        print(json.dumps({T: r}), flush=True)
        if subdiv == 5:
            values, origins = mesh_to_sdf.occupancy(tri, 64, mesh_to_sdf._caster(tri, 'bvh'))
            grid = redistancing.redistance(values)
            cast = bvh.raycast
            res['refine64'] = dict(triangles=T, near_voxels=int((grid.abs() < 1.0 / 64).sum()),
                                   rays_ms=timed(lambda: mesh_to_sdf.refine(tri, grid, origins, 64, cast=cast), 3),
                                   closest_ms=timed(lambda: mesh_to_sdf.refine(tri, grid, origins, 64, distance='closest', accel='bvh'), 3))
            print(json.dumps(res['refine64']), flush=True)
    lines = ['# Closest-point queries on the mesh BVH: timings', '',
             f"`python tools/mesh_closest_bench.py` on {res['device']}: host clock around work that ends in a device synchronise, median (minimum) of "
             f"{a.reps} runs after a warm-up ({max(3, a.reps // 2)} for the brute-force kernel).", "Icospheres of radius 0.3 (queried from the inside too: near the centre of a sphere every triangle is almost equally near and few boxes can be culled -- the hard case of a closest-point search).", '',
             '| triangles | points | n | BVH build ms | BVH query ms | brute force ms | brute / BVH | same bits |', '|---|---|---|---|---|---|---|---|']
    for T, name, n, build, q, b, same in rows:
        lines.append(f'| {T} | {name} | {n} | {build:.3f} | {q[0]:.3f} ({q[1]:.3f}) | {b[0]:.3f} ({b[1]:.3f}) | {b[0] / q[0]:.1f} | {"yes" if same else "NO"} |')
    slower = sorted({T for T, _, _, _, q, b, _ in rows if q[0] > b[0]})
    lines += ['', 'Crossover: ' + (f'the BVH query is slower than brute force at {", ".join(str(t) for t in slower)} triangles (at least one point set).'
                                  if slower else 'the BVH query is faster than brute force at every size measured, the smallest included.'),
              '`mesh_to_sdf.BVH_MIN_TRIANGLES` is left as it is.', '']
    rf = res['refine64']
    lines += [f"`mesh_to_sdf.refine` at 64^3, {rf['triangles']} triangles, {rf['near_voxels']} near-surface voxels, both through the BVH (median (minimum) of 3):", '',
              '| distance | ms |', '|---|---|', f"| 'rays' (256 casts per voxel) | {rf['rays_ms'][0]:.3f} ({rf['rays_ms'][1]:.3f}) |",
              f"| 'closest' (one query per voxel, BVH build included) | {rf['closest_ms'][0]:.3f} ({rf['closest_ms'][1]:.3f}) |", '']
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, 'w') as fh:
        fh.write('\n'.join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
