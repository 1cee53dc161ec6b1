"""`python simplify_mesh.py IN OUT --cells N [--reg r] [--float-colors]`: simplifies any `.ply` / `.obj` triangle mesh by vertex clustering
with quadric error metrics (dsdf.simplify_mesh) at N cells along the longest extent of its bounding box, and writes it with the vertex
normals of the simplified surface.  Vertex colours of the input are averaged per cell and written too (uchar in a ply unless
--float-colors).  mesh_to_sdf.load_mesh_indexed / save_ply / save_obj do the file IO."""
import argparse
import sys

import numpy as np
import torch

import dsdf
import mesh_to_sdf


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('input', help='.ply or .obj triangle mesh')
    ap.add_argument('output', help='.ply (binary) or .obj')
    ap.add_argument('--cells', type=int, required=True, help='cells along the longest extent of the bounding box (cubic cells)')
    ap.add_argument('--reg', type=float, default=dsdf.renderer.SIMPLIFY_REG, help='pull towards the mean of a cell, relative to its area (default 1e-3)')
    ap.add_argument('--float-colors', action='store_true', help='ply: store the colours as float (lossless) instead of uchar')
    args = ap.parse_args(argv)
    if args.cells < 1:
        ap.error('--cells must be >= 1')
    if not args.reg > 0:
        ap.error('--reg must be > 0')
    if not args.output.endswith(('.ply', '.obj')):
        ap.error('the output must be a .ply or an .obj file')
    return args


def main(argv=None):
    args = parse_args(argv)
    v, f, c = mesh_to_sdf.load_mesh_indexed(args.input, colors=True)
    dev = torch.device('cuda')
    vert = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev)
    faces = torch.from_numpy(np.ascontiguousarray(f).astype(np.int32)).to(dev)
    colors = torch.from_numpy(np.ascontiguousarray(c, np.float32)).to(dev) if c is not None else None
    vo, fo, no, *co = dsdf.simplify_mesh(vert, faces, args.cells, normals=True, colors=colors, reg=args.reg)
    co = co[0] if co else None
    if args.output.endswith('.obj'):
        mesh_to_sdf.save_obj(args.output, vo, fo, no, colors=co)
    else:
        mesh_to_sdf.save_ply(args.output, vo, fo, no, colors=co, color_dtype='float' if args.float_colors else 'uchar')
    print(f'{args.output}: {v.shape[0]} -> {vo.shape[0]} vertices, {f.shape[0]} -> {fo.shape[0]} faces')
    return 0


if __name__ == '__main__':
    sys.exit(main())
