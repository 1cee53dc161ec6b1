#!/usr/bin/env python3
"""Times and measures the generalized winding number (csrc/dsdf_winding.h) on the GPU: `python tools/mesh_winding_bench.py [--md FILE] [--out FILE.json]`.

  - query: dsdf.MeshBvh.winding at beta = 2, 3, 4 against the brute-force dsdf.mesh_winding for 1 M random points in [-0.5, 0.5]^3, on
    icospheres of 5 k, 20 k and 82 k triangles, with the largest difference between the two;
  - occupancy: `mesh_to_sdf.occupancy(sign='winding')` against `sign='rays'` (what mesh_to_sdf did before it had a choice) at 128^3 and
    256^3 on the 82 k mesh, both through the BVH, with the number of voxels that differ;
  - errors: the exact sum and the tree at beta = 2, 3, 4 against the fp64 reference (tests/mesh_winding_oracle.py) on the shared meshes of
    the tests, for the device and for the host build of the same statements (tests/harness/dsdf_winding_host.cpp).
Every time is a host clock around work that ends in a device synchronise, the median (and minimum) of `--reps` runs after a warm-up.
It writes the tables to profiles/mesh_winding.md (--md); nothing gates a time."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'differentiable-sdf-rendering_amd', 'python')):
    if p not in sys.path:
        sys.path.insert(0, p)

BETAS = (2.0, 3.0, 4.0)


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
    ap.add_argument('--md', default=os.path.join(ROOT, 'profiles', 'mesh_winding.md'))
    ap.add_argument('--out', default=None)
    ap.add_argument('--points', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=7)
    a = ap.parse_args()
    import numpy as np
    import torch
    import dsdf
    import mesh_oracle as M
    import mesh_to_sdf
    import mesh_winding_oracle as O
    import test_mesh_winding_host as H
    from mesh_bvh_cases import morton_order
    assert torch.cuda.is_available(), "needs a GPU"
    dsdf.load()
    g = torch.Generator(device='cuda').manual_seed(1)
    x = (torch.rand(a.points, 3, device='cuda', generator=g) - 0.5).contiguous()
    res = dict(points=a.points, reps=a.reps, device=torch.cuda.get_device_name(0), meshes={}, occupancy={}, errors={})
    for subdiv in (4, 5, 6):
        v, f = M.icosphere(0.3, subdiv, centre=(0.05, -0.02, 0.01))
        tri = torch.from_numpy(v[f]).cuda()
        T = int(tri.shape[0])
        bvh = dsdf.MeshBvh(tri)

        def moments():
            bvh.moments = None
            bvh.winding(x[:1])
        r = dict(triangles=T, moments_ms=timed(moments, a.reps), brute_ms=timed(lambda: dsdf.mesh_winding(tri, x), 3))
        exact = dsdf.mesh_winding(tri, x)
        for beta in BETAS:
            r[f'beta{beta:g}_ms'] = timed(lambda: bvh.winding(x, beta=beta), a.reps)
            w = bvh.winding(x, beta=beta)
            r[f'beta{beta:g}_max_diff'] = float((w - exact).abs().max())
            r[f'beta{beta:g}_decisions_differ'] = int(((w > 0.5) != (exact > 0.5)).sum())
        res['meshes'][T] = r
        print(json.dumps({T: r}), flush=True)
        if subdiv == 6:
            for n in (128, 256):
                rays = mesh_to_sdf.occupancy(tri, n, bvh.raycast)[0]
                wind = mesh_to_sdf.occupancy(tri, n, sign='winding', accel='bvh')[0]
                o = dict(triangles=T, rays_ms=timed(lambda: mesh_to_sdf.occupancy(tri, n, bvh.raycast), 3),
                         winding_ms=timed(lambda: mesh_to_sdf.occupancy(tri, n, sign='winding', accel='bvh'), 3),
                         voxels_differ=int((rays != wind).sum()))
                res['occupancy'][n] = o
                print(json.dumps({n: o}), flush=True)
    host = H.load_host()
    for name, tri in O.MESHES.items():
        pts, w64 = O.points_and_reference(name)
        tri_d, pts_d = torch.from_numpy(tri).cuda(), torch.from_numpy(pts).cuda()
        bvh = dsdf.MeshBvh(tri_d)
        tree = H.build(host, tri, morton_order(tri))
        err = lambda w: float(np.abs(np.asarray(w, np.float64) - w64).max())
        e = dict(triangles=int(tri.shape[0]), points=int(pts.shape[0]), device_exact=err(dsdf.mesh_winding(tri_d, pts_d).cpu().numpy()),
                 host_exact=err(H.brute(host, tri, pts)))
        for beta in BETAS:
            e[f'device_beta{beta:g}'] = err(bvh.winding(pts_d, beta=beta).cpu().numpy())
            e[f'host_beta{beta:g}'] = err(H.walk(host, tree, pts, beta))
        res['errors'][name] = e
        print(json.dumps({name: e}), flush=True)
    ms = lambda t: f'{t[0]:.3f} ({t[1]:.3f})'
    lines = ['# Generalized winding number: timings and errors', '',
             f"`python tools/mesh_winding_bench.py` on {res['device']}: host clock around work that ends in a device synchronise, median (minimum) of "
             f"{a.reps} runs after a warm-up (3 for the brute-force kernel and the occupancies).", '',
             f'## Query: {a.points} random points in [-0.5, 0.5]^3, icospheres of radius 0.3', '',
             'max diff: the largest |tree - brute force| over the points; flips: points on the other side of 0.5.', '',
             '| triangles | moments ms | brute force ms | ' + ' | '.join(f'beta {b:g} ms | max diff | flips' for b in BETAS) + ' |',
             '|---|---|---|' + '---|---|---|' * len(BETAS)]
    for T, r in res['meshes'].items():
        lines.append(f"| {T} | {ms(r['moments_ms'])} | {ms(r['brute_ms'])} | " + ' | '.join(
            f"{ms(r[f'beta{b:g}_ms'])} | {r[f'beta{b:g}_max_diff']:.2e} | {r[f'beta{b:g}_decisions_differ']}" for b in BETAS) + ' |')
    lines += ['', "## Occupancy: `mesh_to_sdf.occupancy` on the 82 k mesh through the BVH, sign='rays' (two or three ray casts per voxel) against "
              "sign='winding' (beta = 2, moments included)", '', '| grid | rays ms | winding ms | voxels that differ |', '|---|---|---|---|']
    for n, o in res['occupancy'].items():
        lines.append(f"| {n}^3 | {ms(o['rays_ms'])} | {ms(o['winding_ms'])} | {o['voxels_differ']} |")
    lines += ['', '## Errors against the fp64 reference (tests/mesh_winding_oracle.py), shared meshes and points of the tests', '',
              'max |w - w_fp64|; exact: the sum over all triangles; the tree in Morton order.  Host: the g++ build of the same statements '
              '(its largest exact error is `MEASURED_MAX_ERR`).', '',
              '| mesh | triangles | points | exact, host | exact, device | ' + ' | '.join(f'beta {b:g}, host | beta {b:g}, device' for b in BETAS) + ' |',
              '|---|---|---|---|---|' + '---|---|' * len(BETAS)]
    for name, e in res['errors'].items():
        lines.append(f"| {name} | {e['triangles']} | {e['points']} | {e['host_exact']:.3e} | {e['device_exact']:.3e} | " + ' | '.join(
            f"{e[f'host_beta{b:g}']:.3e} | {e[f'device_beta{b:g}']:.3e}" for b in BETAS) + ' |')
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
