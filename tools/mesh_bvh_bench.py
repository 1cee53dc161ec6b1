#!/usr/bin/env python3
"""Times the mesh BVH (csrc/dsdf_bvh.h) on the GPU: `python tools/mesh_bvh_bench.py [--out FILE.json]`.

  - Morton pass + sort + build (dsdf.MeshBvh) for icospheres of 5 k, 20 k and 82 k triangles;
  - 1 M random rays and 1 M camera rays against each, through the BVH and through the brute-force kernel (dsdf.mesh_raycast), with
    the results compared bit for bit;
  - `mesh_to_sdf.create_sdf` at 64^3 both ways (20 k triangles);
  - one 512^2, 64-spp mesh render per integrator (20 k triangles), and the direct one again with corner colours;
  - with `--build-lds` (run where hipcc is; no GPU needed) a second library that stages the top 255 nodes of the tree in LDS
    (-DDSDF_BVH_LDS_NODES=255) is compiled to lib/variants/libdsdf_bvh_lds.so; when that file exists the ray casts are also timed
    through it, alternating with the default build (no staging).
Every time is a host clock around work that ends in a device synchronise, the median of `--reps` runs after a warm-up.
profiles/mesh_bvh.md holds the results."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'differentiable-sdf-rendering_amd', 'python')):
    if p not in sys.path:
        sys.path.insert(0, p)
LDS = os.path.join(ROOT, 'differentiable-sdf-rendering_amd', 'lib', 'variants', 'libdsdf_bvh_lds.so')


def build_lds():
    import __graft_entry__ as g
    return g.build_variant('bvh_lds', ['-DDSDF_BVH_LDS_NODES=255'])


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
    ap.add_argument('--rays', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--build-lds', action='store_true')
    a = ap.parse_args()
    if a.build_lds:
        print(build_lds())
        return
    import numpy as np
    import torch
    import dsdf
    import mesh_oracle as M
    import mesh_to_sdf
    from dsdf import _lib
    from dsdf.renderer import _ptr, _stream
    assert torch.cuda.is_available(), "needs a GPU"
    dsdf.load()
    staged = _lib._open(LDS) if os.path.isfile(LDS) else None
    res = dict(rays=a.rays, reps=a.reps, meshes={})
    n = a.rays
    g = torch.Generator(device='cuda').manual_seed(1)
    ro = torch.rand(n, 3, device='cuda', generator=g) - 0.5
    rd = torch.nn.functional.normalize(torch.randn(n, 3, device='cuda', generator=g), dim=1)
    # camera rays: a 1024 x 1024 pinhole grid from (1.2, 0.9, 1.4) towards the origin, 39 degrees
    side = int(n ** 0.5)
    eye = torch.tensor([1.2, 0.9, 1.4], device='cuda')
    fwd = torch.nn.functional.normalize(-eye, dim=0)
    left = torch.nn.functional.normalize(torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], device='cuda'), fwd), dim=0)
    up = torch.linalg.cross(fwd, left)
    s = (torch.arange(side, device='cuda') + 0.5) / side * 2 - 1
    yy, xx = torch.meshgrid(s, s, indexing='ij')
    tan = float(np.tan(np.radians(39.0) / 2))
    cd = torch.nn.functional.normalize(fwd + tan * (xx.reshape(-1, 1) * left + yy.reshape(-1, 1) * up), dim=1).contiguous()
    co = eye.expand_as(cd).contiguous()

    def cast_with(lib, bvh, o, d, t, back):
        _lib.check(lib.dsdf_mesh_bvh_raycast(_ptr(bvh.buffer), _ptr(o), _ptr(d), o.shape[0], C.c_float(0.0), _ptr(t), _ptr(back), None, _stream()), lib)

    for subdiv in (4, 5, 6):
        v, f = M.icosphere(0.3, subdiv, centre=(0.05, -0.02, 0.01))
        tri = torch.from_numpy(v[f]).cuda()
        T = int(tri.shape[0])
        r = dict(triangles=T)
        r['build_ms'] = timed(lambda: dsdf.MeshBvh(tri), a.reps)
        bvh = dsdf.MeshBvh(tri)
        for name, (o, d) in (('random', (ro, rd)), ('camera', (co, cd))):
            r[f'{name}_bvh_ms'] = timed(lambda: bvh.raycast(o, d), a.reps)
            r[f'{name}_brute_ms'] = timed(lambda: dsdf.mesh_raycast(tri, o, d), max(3, a.reps // 2))
            tb, bb = bvh.raycast(o, d)
            t0, b0 = dsdf.mesh_raycast(tri, o, d)
            r[f'{name}_bitwise_equal'] = bool(torch.equal(tb.view(torch.int32), t0.view(torch.int32)) and torch.equal(bb, b0))
            r[f'{name}_hit_fraction'] = float(torch.isfinite(tb).float().mean())
            r[f'{name}_speedup_with_build'] = r[f'{name}_brute_ms'][0] / (r[f'{name}_bvh_ms'][0] + r['build_ms'][0])
            if staged is not None:                            # interleaved A/B of the two builds of the traversal kernel
                t = torch.empty(o.shape[0], device='cuda'); back = torch.empty(o.shape[0], dtype=torch.int32, device='cuda')
                ab = {'lds': [], 'nolds': []}
                for lib in (_lib.load(), staged):
                    cast_with(lib, bvh, o, d, t, back)
                torch.cuda.synchronize()
                for _ in range(a.reps):
                    for tag, lib in (('nolds', _lib.load()), ('lds', staged)):
                        t0_ = time.perf_counter()
                        cast_with(lib, bvh, o, d, t, back)
                        torch.cuda.synchronize()
                        ab[tag].append((time.perf_counter() - t0_) * 1e3)
                r[f'{name}_lds_prefix_ms'] = (statistics.median(ab['lds']), min(ab['lds']))
                r[f'{name}_no_prefix_ms'] = (statistics.median(ab['nolds']), min(ab['nolds']))
        res['meshes'][T] = r
        print(json.dumps({T: r}), flush=True)
        if subdiv == 5:
            for accel in ('bvh', 'brute'):
                res[f'create_sdf64_{accel}_ms'] = timed(lambda: mesh_to_sdf.create_sdf(tri, 64, accel=accel), 3)
            sen = dsdf.get_regular_cameras(1, resx=512, resy=512)[0]
            tri_u = tri + 0.5
            import scenes
            nrm = torch.from_numpy(mesh_to_sdf.vertex_normals(v + np.float32(0.5), f)).cuda()
            rb = dsdf.MeshBvh(tri_u, nrm)
            sh = dsdf.Shading(scenes.load_target_albedo('bench', device='cuda'), 1.0)
            for integ in ('sdf_silhouette_reparam', 'sdf_simple_shading_reparam', 'sdf_direct_reparam'):
                res[f'render512_spp64_{integ}_ms'] = timed(lambda: dsdf.mesh_render(rb, [sen], 64, seeds=[3], integrator=integ,
                                                                                   shading=sh if 'direct' in integ else None), a.reps)
            # the same render with a reflectance per triangle corner (the volume's value at the corners) instead of the volume lookup
            cb = dsdf.MeshBvh(tri_u, nrm, colors=dsdf.sample_volume(sh.albedo, tri_u.reshape(-1, 3)).reshape(-1, 3, 3))
            res['render512_spp64_sdf_direct_reparam_colors_ms'] = timed(lambda: dsdf.mesh_render(cb, [sen], 64, seeds=[3], integrator='sdf_direct_reparam',
                                                                                              shading=dsdf.Shading(None, 1.0)), a.reps)
            print(json.dumps({k: v_ for k, v_ in res.items() if k.startswith(('create', 'render'))}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
