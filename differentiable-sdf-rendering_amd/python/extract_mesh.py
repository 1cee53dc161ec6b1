"""`python extract_mesh.py <file.vol> [-o out.ply|out.obj] [--res N] [--iso v] [--albedo <file.vol> [--float-colors]] [--keep-largest [K]]
[--min-component-area A] [--simplify N]`: the triangle mesh of the surface the renderer sees in an SDF checkpoint (the `.vol` files optimize.py writes) -- dsdf.extract_mesh on util.read_vol,
written by mesh_to_sdf.save_ply / save_obj with the vertex normals.  The mesh lives in the unit cube of the grid, like the SDF.
--albedo: the reflectance checkpoint of a textured reconstruction (three channels); its value at every vertex is written as the vertex
colour (linear, no gamma) -- uchar in a ply unless --float-colors.
--simplify N: the extracted mesh goes through dsdf.simplify_mesh at N cells along its longest extent before it is written (vertex
clustering with quadric errors: a much lighter file whose surface stays where the full-resolution extraction put it); normals and
colours are carried through.
--keep-largest [K] (1 when no number follows), --min-component-area A: only the K connected components of largest area, and only those of
at least area A, are written (dsdf.filter_components) -- what removes the floaters an optimisation leaves away from the object.  They
apply after the extraction and before --simplify."""
import argparse
import os
import sys

import dsdf
import mesh_to_sdf
import util


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('vol', help='SDF grid as a Mitsuba volume file (one channel)')
    ap.add_argument('-o', '--output', default=None, help='.ply (binary) or .obj; default: the input name with .ply')
    ap.add_argument('--res', type=int, default=None, help="cells per axis of the extraction lattice (default: the grid's own resolution)")
    ap.add_argument('--iso', type=float, default=0.0, help='level to extract (default 0)')
    ap.add_argument('--steps', type=int, default=24, help='bisection steps per vertex (1 ... 32)')
    ap.add_argument('--albedo', default=None, help='reflectance volume (three channels): baked onto the vertices as vertex colours')
    ap.add_argument('--simplify', type=int, default=None, metavar='N',
                    help='simplify the mesh by vertex clustering at N cells along its longest extent (dsdf.simplify_mesh)')
    ap.add_argument('--float-colors', action='store_true', help='ply: store the colours as float (lossless) instead of uchar')
    ap.add_argument('--keep-largest', type=int, nargs='?', const=1, default=None, metavar='K',
                    help='keep only the K connected components of largest area (1 when no number follows)')
    ap.add_argument('--min-component-area', type=float, default=None, metavar='A', help='drop connected components of less area than A')
    return ap


def parse_args(argv=None, ap=None):
    ap = ap or parser()
    args = ap.parse_args(argv)
    if args.simplify is not None and args.simplify < 1:
        ap.error('--simplify needs a cell count >= 1')
    if args.keep_largest is not None and args.keep_largest < 1:
        ap.error('--keep-largest needs a count >= 1')
    if args.min_component_area is not None and not args.min_component_area >= 0:
        ap.error('--min-component-area must be >= 0')
    return args


def main(argv=None):
    ap = parser()
    args = parse_args(argv, ap)
    out = args.output or os.path.splitext(args.vol)[0] + '.ply'
    if not out.endswith(('.ply', '.obj')):
        ap.error('the output must be a .ply or an .obj file')
    data = util.read_vol(args.vol)
    if data.dim() != 3:
        ap.error(f'{args.vol}: expected a one-channel volume, got shape {tuple(data.shape)}')
    grid = dsdf.SdfGrid(data.float().contiguous())
    albedo = None
    if args.albedo is not None:
        albedo = util.read_vol(args.albedo)
        if albedo.dim() != 4 or albedo.shape[3] != 3:
            ap.error(f'{args.albedo}: expected a three-channel volume, got shape {tuple(albedo.shape)}')
        albedo = albedo.float().contiguous()
    v, f, n, *c = dsdf.extract_mesh(grid, resolution=args.res, iso=args.iso, steps=args.steps, colors=albedo)
    c = c[0] if c else None
    if args.keep_largest is not None or args.min_component_area is not None:
        full = f.shape[0]
        v, f, n, *c, (found, kept) = dsdf.filter_components(v, f, keep=args.keep_largest, min_area=args.min_component_area, normals=n, colors=c,
                                                           return_counts=True)
        c = c[0] if c else None
        print(f'components: {found} found, {kept} kept, {full} -> {f.shape[0]} faces')
    if args.simplify is not None and f.shape[0] > 0:
        full = f.shape[0]
        v, f, n, *c = dsdf.simplify_mesh(v, f, args.simplify, normals=True, colors=c)
        c = c[0] if c else None
        print(f'simplified at {args.simplify} cells: {full} -> {f.shape[0]} faces')
    if out.endswith('.obj'):
        mesh_to_sdf.save_obj(out, v, f, n, colors=c)
    else:
        mesh_to_sdf.save_ply(out, v, f, n, colors=c, color_dtype='float' if args.float_colors else 'uchar')
    print(f'{out}: {v.shape[0]} vertices, {f.shape[0]} faces')
    return 0


if __name__ == '__main__':
    sys.exit(main())
