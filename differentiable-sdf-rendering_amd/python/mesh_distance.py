"""`python mesh_distance.py A B [--samples N] [--seed S] [--threshold T] [--res N] [--largest-component] [--json FILE]`: how far two surfaces are apart --
Chamfer and Hausdorff distance, and precision / recall / F-score at a threshold (dsdf.mesh_distance: points sampled on each surface,
the closest point of the other through its BVH).  A and B are `.ply` / `.obj` meshes (mesh_to_sdf.load_mesh) or `.vol` SDF checkpoints
(the files optimize.py writes), whose surface is first extracted with dsdf.extract_mesh on a lattice of --res cells.  Meshes live in
the scene's frame, [-0.5, 0.5]^3; an extracted one lives in the unit cube of its grid (what extract_mesh.py writes) and is shifted by
-0.5 into that frame, the inverse of where mesh_to_sdf.create_sdf puts the voxel centres.  A is the reconstruction and B the target
in `precision` (the share of A within T of B) and `recall` (the share of B within T of A)."""
import argparse
import json
import sys

import numpy as np
import torch

import dsdf
import mesh_to_sdf
import util

METRICS = ('a_to_b_mean', 'b_to_a_mean', 'a_to_b_max', 'b_to_a_max', 'chamfer_l1', 'chamfer_l2', 'hausdorff', 'precision', 'recall', 'fscore')


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('a', help='.ply / .obj mesh, or .vol SDF checkpoint')
    ap.add_argument('b', help='.ply / .obj mesh, or .vol SDF checkpoint')
    ap.add_argument('--samples', type=int, default=200_000, help='points sampled on each surface (default 200000)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--threshold', type=float, default=None, help='distance for precision / recall / F-score')
    ap.add_argument('--res', type=int, default=None, help="cells per axis when a .vol is extracted (default: the grid's own resolution)")
    ap.add_argument('--largest-component', action='store_true',
                    help='score only the connected component of largest area of each input (drops floaters before sampling)')
    ap.add_argument('--json', default=None, help='also write the metrics to this file')
    args = ap.parse_args(argv)
    for fn in (args.a, args.b):
        if not fn.endswith(('.ply', '.obj', '.vol')):
            ap.error(f'{fn}: expected a .ply, .obj or .vol file')
    if args.samples < 1:
        ap.error('--samples must be positive')
    return args


def load_surface(fn, res=None, device='cuda', largest_component=False):
    """(T, 3, 3) float32 device triangles of a mesh file, or of the surface of a .vol checkpoint, in the scene's frame.
    largest_component: only the connected component of largest area (dsdf.filter_components; the vertices of a file are merged by
    position first, so that a file which repeats its vertices per face does not fall apart into single triangles)."""
    if not fn.endswith('.vol'):
        if not largest_component:
            return torch.from_numpy(mesh_to_sdf.load_mesh(fn)).to(device).contiguous()
        v, f = mesh_to_sdf.load_mesh_indexed(fn)
        v, f = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(device), torch.from_numpy(np.ascontiguousarray(f).astype(np.int32)).to(device)
        v, f = dsdf.filter_components(v, f, keep=1, connect='position')
        return v[f.long()].contiguous()
    data = util.read_vol(fn)
    if data.dim() != 3:
        raise ValueError(f'{fn}: expected a one-channel volume, got shape {tuple(data.shape)}')
    v, f = dsdf.extract_mesh(dsdf.SdfGrid(data.float().contiguous()), resolution=res, normals=False)
    if f.shape[0] == 0:
        raise ValueError(f'{fn}: the grid has no surface')
    if largest_component:
        v, f = dsdf.filter_components(v, f, keep=1)
    return (v - 0.5)[f.long()].contiguous()


def main(argv=None):
    args = parse_args(argv)
    a, b = (load_surface(fn, args.res, largest_component=args.largest_component) for fn in (args.a, args.b))
    res = dsdf.mesh_distance(a, b, n=args.samples, seed=args.seed, threshold=args.threshold)
    out = {k: res[k] for k in METRICS if k in res}
    for k, v in out.items():
        print(f'{k}: {v:.9g}')
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
