"""`python mesh_components.py IN [-o OUT] [--keep-largest K] [--min-area A] [--min-faces N] [--connect index|position] [--json FILE]`: lists
the connected components of a triangle mesh (dsdf.mesh_components) -- faces, area, signed volume, closed or open, bounding box -- and with
-o writes the mesh without the components that the three filters drop (dsdf.filter_components); the vertex colours of a mesh file and
the vertex normals of an extraction stay with their vertices.
IN is a `.ply` / `.obj` mesh (mesh_to_sdf.load_mesh_indexed), or a `.vol` SDF checkpoint whose surface is first extracted with
dsdf.extract_mesh on a lattice of --res cells, as mesh_distance.py does.  --connect position first merges vertices with equal
coordinates: for files that repeat their vertices per face.  The volume of an open component depends on where the origin is and is
listed for completeness only."""
import argparse
import json
import sys

import numpy as np
import torch

import dsdf
import mesh_to_sdf
import util


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('input', help='.ply / .obj mesh, or .vol SDF checkpoint')
    ap.add_argument('-o', '--output', default=None, help='.ply (binary) or .obj: the mesh without the components filtered away')
    ap.add_argument('--keep-largest', type=int, default=None, metavar='K', help='keep only the K components of largest area')
    ap.add_argument('--min-area', type=float, default=None, metavar='A', help='drop components of less area than A')
    ap.add_argument('--min-faces', type=int, default=None, metavar='N', help='drop components of fewer than N faces')
    ap.add_argument('--connect', choices=('index', 'position'), default='index', help="'position' merges vertices with equal coordinates first")
    ap.add_argument('--res', type=int, default=None, help="cells per axis when a .vol is extracted (default: the grid's own resolution)")
    ap.add_argument('--float-colors', action='store_true', help='ply: store the colours as float (lossless) instead of uchar')
    ap.add_argument('--json', default=None, help='also write the list of components to this file')
    args = ap.parse_args(argv)
    if not args.input.endswith(('.ply', '.obj', '.vol')):
        ap.error(f'{args.input}: expected a .ply, .obj or .vol file')
    if args.output is not None and not args.output.endswith(('.ply', '.obj')):
        ap.error('the output must be a .ply or an .obj file')
    if args.keep_largest is not None and args.keep_largest < 1:
        ap.error('--keep-largest must be >= 1')
    if args.min_area is not None and not args.min_area >= 0:
        ap.error('--min-area must be >= 0')
    if args.min_faces is not None and args.min_faces < 0:
        ap.error('--min-faces must be >= 0')
    return args


def load_indexed(fn, res=None, device='cuda'):
    """(vertices, faces, normals or None, colors or None) on the device: a mesh file as it is, a .vol through dsdf.extract_mesh."""
    if fn.endswith('.vol'):
        data = util.read_vol(fn)
        if data.dim() != 3:
            raise ValueError(f'{fn}: expected a one-channel volume, got shape {tuple(data.shape)}')
        v, f, n = dsdf.extract_mesh(dsdf.SdfGrid(data.float().contiguous()), resolution=res)
        return v, f, n, None
    v, f, c = mesh_to_sdf.load_mesh_indexed(fn, colors=True)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(device)
    return up(v, np.float32), up(f, np.int32), None, up(c, np.float32) if c is not None else None


def main(argv=None):
    args = parse_args(argv)
    v, f, n, c = load_indexed(args.input, args.res)
    comp = dsdf.mesh_components(f, vertices=v, connect=args.connect)
    rows = [dict(component=i, faces=int(nf), area=float(a), volume=float(w), closed=int(b) == 0, boundary_edges=int(b), bbox=box)
            for i, (nf, a, w, b, box) in enumerate(zip(comp.faces_per_component.tolist(), comp.area.tolist(), comp.volume.tolist(),
                                                       comp.boundary_edges.tolist(), comp.bbox.tolist()))]
    print(f'{args.input}: {v.shape[0]} vertices, {f.shape[0]} faces, {comp.n} components')
    for r in rows:
        lo, hi = r['bbox']
        print(f"{r['component']:6d}: {r['faces']:8d} faces, area {r['area']:.6g}, volume {r['volume']:.6g}, "
              f"{'closed' if r['closed'] else 'open (' + str(r['boundary_edges']) + ' boundary edges)'}, "
              f"bbox [{lo[0]:.4g}, {lo[1]:.4g}, {lo[2]:.4g}] - [{hi[0]:.4g}, {hi[1]:.4g}, {hi[2]:.4g}]")
    result = dict(vertices=int(v.shape[0]), faces=int(f.shape[0]), components=rows)
    if args.output is not None:
        extras = dict(normals=n, colors=c)
        vo, fo, *rest, (found, kept) = dsdf.filter_components(v, f, keep=args.keep_largest, min_area=args.min_area, min_faces=args.min_faces,
                                                              connect=args.connect, return_counts=True, **extras)
        no = rest.pop(0) if n is not None else None
        co = rest.pop(0) if c is not None else None
        print(f'components: {found} found, {kept} kept, {f.shape[0]} -> {fo.shape[0]} faces')
        if args.output.endswith('.obj'):
            mesh_to_sdf.save_obj(args.output, vo, fo, no, colors=co)
        else:
            mesh_to_sdf.save_ply(args.output, vo, fo, no, colors=co, color_dtype='float' if args.float_colors else 'uchar')
        print(f'{args.output}: {vo.shape[0]} vertices, {fo.shape[0]} faces')
        result.update(kept=kept, faces_out=int(fo.shape[0]), vertices_out=int(vo.shape[0]))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(result, fh, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
