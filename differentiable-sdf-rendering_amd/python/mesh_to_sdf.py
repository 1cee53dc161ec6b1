"""`create_sdf(mesh_fn, resolution, refine_surface=True)` (python/mesh_to_sdf.py:9-57): watertight mesh -> SDF grid by
ray casting and redistancing.  The reference takes the ray casts from Mitsuba (`scene.ray_intersect` on an obj / ply
shape) and the redistancing from `fastsweep`; here both are libdsdf.so entry points (`dsdf_mesh_raycast`,
`dsdf_redistance`).  Returns a (res, res, res) float32 CUDA tensor indexed [z, y, x] over [0,1]^3 voxel centres shifted
to [-0.5, 0.5]^3, exactly the reference's placement (:20-22: the mesh is expected inside that cube).
"""
import math
import struct

import numpy as np
import torch

import dsdf
import redistancing

ANGULAR_RES = 16            # mesh_to_sdf.py:40: 16 x 16 stratified directions per near-surface voxel
BVH_MIN_TRIANGLES = dsdf.renderer.BVH_MIN_TRIANGLES    # (4096) accel=None: meshes above this go through dsdf.MeshBvh, smaller ones through the brute-force kernel


def load_obj(fn, colors=False):
    """Vertices / faces of a Wavefront obj (positions only; polygons are fan-triangulated, negative indices resolved).  colors: a third
    element, the (V, 3) float32 vertex colours of `v x y z r g b` lines, or None unless every vertex carries one."""
    v, f, c = [], [], []
    with open(fn) as fh:
        for line in fh:
            s = line.split()
            if not s:
                continue
            if s[0] == 'v':
                v.append([float(s[1]), float(s[2]), float(s[3])])
                if len(s) >= 7:
                    c.append([float(s[4]), float(s[5]), float(s[6])])
            elif s[0] == 'f':
                idx = []
                for tok in s[1:]:
                    k = int(tok.split('/')[0])
                    idx.append(k - 1 if k > 0 else len(v) + k)
                for j in range(1, len(idx) - 1):
                    f.append([idx[0], idx[j], idx[j + 1]])
    v, f = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    if not colors:
        return v, f
    return v, f, (np.asarray(c, np.float32).reshape(-1, 3) if len(c) == len(v) and len(v) else None)


_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def _ply_color_scale(type_name):
    """What a stored colour component is divided by: an integer type spans [0, max], a float type is the value itself."""
    dt = np.dtype(_PLY_TYPES[type_name])
    return float(np.iinfo(dt).max) if dt.kind in 'iu' else 1.0


def load_ply(fn, colors=False):
    """Vertices / faces of a ply file (ascii, binary_little_endian or binary_big_endian; x y z + one index list per face).  colors: a
    third element, the (V, 3) float32 vertex colours of the properties `red green blue` (uchar divided by 255, float as stored), or
    None when the file has none."""
    with open(fn, 'rb') as fh:
        if fh.readline().strip() != b'ply':
            raise ValueError(f'{fn}: not a ply file')
        fmt, elements = None, []
        while True:
            line = fh.readline()
            if not line:
                raise ValueError(f'{fn}: truncated ply header')
            s = line.decode('ascii', 'replace').split()
            if not s or s[0] == 'comment':
                continue
            if s[0] == 'format':
                fmt = s[1]
            elif s[0] == 'element':
                elements.append((s[1], int(s[2]), []))
            elif s[0] == 'property':
                elements[-1][2].append(tuple(s[1:]))
            elif s[0] == 'end_header':
                break
        if fmt not in ('ascii', 'binary_little_endian', 'binary_big_endian'):
            raise ValueError(f'{fn}: unsupported ply format {fmt}')
        en = '>' if fmt == 'binary_big_endian' else '<'
        verts, faces, cols = None, [], None
        tokens = None
        if fmt == 'ascii':
            tokens = iter(fh.read().split())
        for name, count, props in elements:
            has_list = any(p[0] == 'list' for p in props)
            if fmt == 'ascii':
                rows = []
                for _ in range(count):
                    row = []
                    for p in props:
                        if p[0] == 'list':
                            k = int(next(tokens))
                            row.append([int(float(next(tokens))) for _ in range(k)])
                        else:
                            row.append(float(next(tokens)))
                    rows.append(row)
            elif not has_list:
                dt = np.dtype([(p[1], en + _PLY_TYPES[p[0]]) for p in props])
                arr = np.frombuffer(fh.read(dt.itemsize * count), dtype=dt, count=count)
                rows = arr
            else:
                rows = []
                for _ in range(count):
                    row = []
                    for p in props:
                        if p[0] == 'list':
                            ct, it = np.dtype(en + _PLY_TYPES[p[1]]), np.dtype(en + _PLY_TYPES[p[2]])
                            k = int(np.frombuffer(fh.read(ct.itemsize), ct)[0])
                            row.append(np.frombuffer(fh.read(it.itemsize * k), it).astype(np.int64).tolist())
                        else:
                            t = np.dtype(en + _PLY_TYPES[p[0]])
                            row.append(float(np.frombuffer(fh.read(t.itemsize), t)[0]))
                    rows.append(row)
            if name == 'vertex':
                names = [p[-1] for p in props]
                if isinstance(rows, np.ndarray):
                    verts = np.stack([rows['x'], rows['y'], rows['z']], -1).astype(np.float32)
                else:
                    ix = [names.index(c) for c in 'xyz']
                    verts = np.asarray([[r[i] for i in ix] for r in rows], np.float32).reshape(-1, 3)
                if all(c in names for c in ('red', 'green', 'blue')):
                    chans = []
                    for c in ('red', 'green', 'blue'):
                        i = names.index(c)
                        col = rows[c] if isinstance(rows, np.ndarray) else np.asarray([r[i] for r in rows], np.float64)
                        chans.append(col.astype(np.float64) / _ply_color_scale(props[i][0]))
                    cols = np.stack(chans, -1).astype(np.float32).reshape(-1, 3)
            elif name == 'face':
                li = [i for i, p in enumerate(props) if p[0] == 'list'][0]
                for r in rows:
                    idx = r[li]
                    for j in range(1, len(idx) - 1):
                        faces.append([idx[0], idx[j], idx[j + 1]])
        if verts is None:
            raise ValueError(f'{fn}: no vertex element')
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return (verts, faces, cols) if colors else (verts, faces)


def _mesh_arrays(vertices, faces, normals, colors=None):
    def host(a, dt):
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        return np.ascontiguousarray(a, dt).reshape(-1, 3)
    v, f = host(vertices, '<f4'), host(faces, '<i4')
    n = host(normals, '<f4') if normals is not None else None
    if n is not None and n.shape != v.shape:
        raise ValueError(f'normals must be (V, 3) like vertices, got {n.shape}')
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError('face index out of range')
    if colors is None:
        return v, f, n
    c = colors.detach().cpu().numpy() if torch.is_tensor(colors) else np.asarray(colors)
    if c.shape != v.shape:
        raise ValueError(f'colors must be (V, 3) like vertices, got {c.shape}')
    return v, f, n, np.ascontiguousarray(c, '<f4')


def save_ply(fn, vertices, faces, normals=None, colors=None, color_dtype='uchar'):
    """Writes an indexed triangle mesh (what dsdf.extract_mesh returns: tensors or arrays) as binary little-endian ply: x y z
    [nx ny nz] [red green blue] per vertex, one uchar-counted int list per face.  load_ply reads it back.
    colors (V, 3): LINEAR reflectance, written as it is -- no gamma is applied, a viewer that expects sRGB shows it darker.
    color_dtype 'uchar' stores round(clip(c, 0, 1) * 255), what mesh viewers read; 'float' stores the values losslessly."""
    if color_dtype not in ('uchar', 'float'):
        raise ValueError(f"color_dtype must be 'uchar' or 'float', got {color_dtype!r}")
    c = None
    if colors is None:
        v, f, n = _mesh_arrays(vertices, faces, normals)
    else:
        v, f, n, c = _mesh_arrays(vertices, faces, normals, colors)
    fields = [('p', '<f4', (3,))] + ([('n', '<f4', (3,))] if n is not None else [])
    props = [f'property float {k}' for k in ['x', 'y', 'z'] + (['nx', 'ny', 'nz'] if n is not None else [])]
    if c is not None:
        fields.append(('c', 'u1' if color_dtype == 'uchar' else '<f4', (3,)))
        props += [f'property {color_dtype} {k}' for k in ('red', 'green', 'blue')]
    head = ['ply', 'format binary_little_endian 1.0', f'element vertex {len(v)}'] + props + \
           [f'element face {len(f)}', 'property list uchar int vertex_indices', 'end_header']
    vrec = np.zeros(len(v), np.dtype(fields))
    vrec['p'] = v
    if n is not None:
        vrec['n'] = n
    if c is not None:
        vrec['c'] = np.rint(np.clip(c.astype(np.float64), 0.0, 1.0) * 255.0).astype('u1') if color_dtype == 'uchar' else c
    rec = np.zeros(len(f), np.dtype([('k', 'u1'), ('i', '<i4', (3,))]))
    rec['k'] = 3
    rec['i'] = f
    with open(fn, 'wb') as fh:
        fh.write(('\n'.join(head) + '\n').encode('ascii'))
        fh.write(vrec.tobytes())
        fh.write(rec.tobytes())
    return fn


def save_obj(fn, vertices, faces, normals=None, colors=None):
    """The same mesh as a Wavefront obj (v [vn] f, 1-based; 9 significant digits: float32 round-trips).  load_obj reads it back.
    colors (V, 3): linear reflectance (no gamma), written as `v x y z r g b`."""
    c = None
    if colors is None:
        v, f, n = _mesh_arrays(vertices, faces, normals)
    else:
        v, f, n, c = _mesh_arrays(vertices, faces, normals, colors)
    with open(fn, 'w') as fh:
        if c is not None:
            fh.writelines('v %.9g %.9g %.9g %.9g %.9g %.9g\n' % tuple(r) for r in np.concatenate([v, c], 1).tolist())
        else:
            fh.writelines('v %.9g %.9g %.9g\n' % tuple(r) for r in v.tolist())
        if n is not None:
            fh.writelines('vn %.9g %.9g %.9g\n' % tuple(r) for r in n.tolist())
            fh.writelines('f %d//%d %d//%d %d//%d\n' % (a, a, b, b, c, c) for a, b, c in (f + 1).tolist())
        else:
            fh.writelines('f %d %d %d\n' % tuple(r) for r in (f + 1).tolist())
    return fn


def load_mesh_indexed(mesh_fn, colors=False):
    """(V, 3) float32 vertices and (T, 3) faces; the plugin is chosen the way the reference does (mesh_to_sdf.py:12).  colors: a third
    element, the (V, 3) float32 vertex colours of the file, or None when it has none."""
    v, f, c = load_obj(mesh_fn, True) if mesh_fn.endswith('.obj') else load_ply(mesh_fn, True)
    if len(f) == 0:
        raise ValueError(f'{mesh_fn}: no faces')
    return (v, f, c) if colors else (v, f)


def load_mesh(mesh_fn):
    """(T, 3, 3) float32 triangle corners."""
    v, f = load_mesh_indexed(mesh_fn)
    return v[f]


def vertex_normals(v, f, smooth=True):
    """(T, 3, 3) float32 normals at the corners of every triangle.  smooth: angle-weighted vertex normals (what Mitsuba computes
    for a mesh file that carries none); otherwise every corner takes its triangle's face normal."""
    p = np.asarray(v, np.float64)[f]
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-300)
    if not smooth:
        return np.repeat(fn[:, None, :], 3, 1).astype(np.float32)
    vn = np.zeros((len(v), 3))
    for k in range(3):
        a, b = p[:, (k + 1) % 3] - p[:, k], p[:, (k + 2) % 3] - p[:, k]
        cosang = (a * b).sum(1) / np.maximum(np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1), 1e-300)
        np.add.at(vn, f[:, k], fn * np.arccos(np.clip(cosang, -1.0, 1.0))[:, None])
    vn /= np.maximum(np.linalg.norm(vn, axis=1, keepdims=True), 1e-300)
    return vn[f].astype(np.float32)


def voxel_centres(res, device):
    """(res^3, 3) points (x, y, z), x fastest -- mesh_to_sdf.py:20-22."""
    c = torch.linspace(-0.5 + 0.5 / res, 0.5 - 0.5 / res, res, dtype=torch.float32, device=device)
    z, y, x = torch.meshgrid(c, c, c, indexing='ij')
    return torch.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], -1).contiguous()


def sphere_directions(device, angular_res=ANGULAR_RES):
    """The angular_res^2 stratified directions of mesh_to_sdf.py:40-45 (`mi.warp.square_to_uniform_sphere` of cell centres)."""
    r = (torch.arange(angular_res, dtype=torch.float32, device=device) + 0.5) / angular_res
    v, u = torch.meshgrid(r, r, indexing='ij')                   # dr.meshgrid default: the first argument varies fastest
    u, v = u.reshape(-1), v.reshape(-1)
    zc = 1.0 - 2.0 * v
    rad = torch.sqrt(torch.clamp(1.0 - zc * zc, min=0.0))
    phi = 2.0 * math.pi * u
    return torch.stack([rad * torch.cos(phi), rad * torch.sin(phi), zc], -1).contiguous()


def _caster(triangles, accel=None):
    """(rays_o, rays_d) -> (t, backface) for this mesh.  accel: 'brute' = dsdf.mesh_raycast, every ray against every triangle;
    'bvh' = dsdf.MeshBvh; None = the BVH above BVH_MIN_TRIANGLES triangles.  Both give the same bits."""
    if accel not in (None, 'bvh', 'brute'):
        raise ValueError(f"accel must be None, 'bvh' or 'brute', got {accel!r}")
    if accel == 'bvh' or (accel is None and triangles.shape[0] > BVH_MIN_TRIANGLES):
        return dsdf.MeshBvh(triangles).raycast
    return lambda o, d: dsdf.mesh_raycast(triangles, o, d)


def _winder(triangles, accel=None):
    """points -> winding number of this mesh.  accel as in _caster: 'brute' = dsdf.mesh_winding (the exact sum), 'bvh' =
    dsdf.MeshBvh.winding (beta = 2: within 0.1 of it), None = the BVH above BVH_MIN_TRIANGLES triangles."""
    if accel not in (None, 'bvh', 'brute'):
        raise ValueError(f"accel must be None, 'bvh' or 'brute', got {accel!r}")
    if accel == 'bvh' or (accel is None and triangles.shape[0] > BVH_MIN_TRIANGLES):
        return dsdf.MeshBvh(triangles).winding
    return lambda x: dsdf.mesh_winding(triangles, x)


def _check_sign(sign):
    if sign not in ('rays', 'winding'):
        raise ValueError(f"sign must be 'rays' or 'winding', got {sign!r}")


def occupancy(triangles, res, cast=None, sign='rays', accel=None):
    """0.5 - inside, inside = the +y ray from the voxel centre leaves the solid through its first hit (mesh_to_sdf.py:23-27).
    The reference casts that one ray with Embree / OptiX, whose intersectors are edge-consistent; dsdf_mesh_raycast tests every
    triangle on its own (Moeller-Trumbore), so a ray through a shared edge or vertex -- voxel centres sit on the symmetry planes
    of many meshes -- can slip between two triangles.  The -y ray answers the same question (a watertight mesh is left
    through a back face in every direction); where the two disagree a third, generic direction decides.
    sign='winding' (opt-in; 'rays' is the reference's method and needs a watertight, consistently oriented mesh without
    self-intersections): inside = the generalized winding number of the voxel centre exceeds 0.5 (_winder(triangles, accel); `cast` is
    not used) -- a mesh with holes or overlapping parts gets the sign a ray would leak along its direction."""
    _check_sign(sign)
    dev = triangles.device
    o = voxel_centres(res, dev)
    if sign == 'winding':
        inside = _winder(triangles, accel)(o) > 0.5
        return (0.5 - inside.float()).reshape(res, res, res), o
    cast = cast or _caster(triangles, 'brute')

    def inside_along(direction):
        d = torch.tensor(direction, dtype=torch.float32, device=dev).expand_as(o).contiguous()
        t, back = cast(o, d)
        return torch.isfinite(t) & (back != 0)
    up, down = inside_along((0.0, 1.0, 0.0)), inside_along((0.0, -1.0, 0.0))
    inside = up
    split = up != down
    if bool(split.any()):
        n = (0.2718 ** 2 + 0.5772 ** 2 + 0.7071 ** 2) ** 0.5
        inside = torch.where(split, inside_along((0.2718 / n, 0.5772 / n, 0.7071 / n)), up)
    return (0.5 - inside.float()).reshape(res, res, res), o


def _nearest(triangles, accel=None):
    """points -> distance to this mesh (one closest-point query each).  accel as in _caster: 'brute' = dsdf.mesh_closest, 'bvh' =
    dsdf.MeshBvh.closest, None = the BVH above BVH_MIN_TRIANGLES triangles.  Both give the same bits."""
    if accel not in (None, 'bvh', 'brute'):
        raise ValueError(f"accel must be None, 'bvh' or 'brute', got {accel!r}")
    if accel == 'bvh' or (accel is None and triangles.shape[0] > BVH_MIN_TRIANGLES):
        return dsdf.MeshBvh(triangles).closest
    return lambda x: dsdf.mesh_closest(triangles, x)


def _check_distance(distance):
    if distance not in ('rays', 'closest'):
        raise ValueError(f"distance must be 'rays' or 'closest', got {distance!r}")


def refine(triangles, grid, origins, res, chunk=1 << 16, cast=None, distance='rays', accel=None):
    """Near-surface voxels (|phi| < 1/res) take the minimum hit distance over the sphere directions, signed by the
    redistanced occupancy (mesh_to_sdf.py:32-55).  No hit in any direction keeps the reference's 100.0.
    distance='closest' (opt-in; 'rays' is the reference's method): |d| of those voxels is instead the exact distance to the mesh, one
    closest-point query per voxel (_nearest(triangles, accel)) in place of 256 ray casts whose minimum is only an upper bound of it; the
    sign is taken from the redistanced occupancy in the same way."""
    _check_distance(distance)
    if distance == 'closest':
        nearest = _nearest(triangles, accel)
        flat = grid.reshape(-1).clone()
        near = torch.nonzero(flat.abs() < 1.0 / res).reshape(-1)
        md = nearest(origins[near].contiguous())
        flat[near] = torch.where(flat[near] < 0, -md, md)        # dr.sign(0) = +1
        return flat.reshape(res, res, res)
    cast = cast or _caster(triangles, 'brute')
    flat = grid.reshape(-1).clone()
    near = torch.nonzero(flat.abs() < 1.0 / res).reshape(-1)
    dirs = sphere_directions(flat.device)
    nd = dirs.shape[0]
    for s in range(0, near.numel(), chunk):
        idx = near[s:s + chunk]
        o = origins[idx].repeat_interleave(nd, 0)
        d = dirs.repeat(idx.numel(), 1)
        t, _ = cast(o, d)
        md = torch.clamp(t.reshape(-1, nd).min(1).values, max=100.0)
        flat[idx] = torch.where(flat[idx] < 0, -md, md)          # dr.sign(0) = +1
    return flat.reshape(res, res, res)


def create_sdf(mesh_fn, resolution, refine_surface=True, device='cuda', accel=None, distance='rays', sign='rays'):
    """Convert a watertight mesh to an SDF using ray casting and redistancing.  `mesh_fn`: path of an obj / ply file, or a
    (T, 3, 3) tensor / array of triangle corners.  accel: how the rays are cast (_caster); the result does not depend on it.
    distance: how `refine` measures the near-surface voxels -- 'rays' (the reference's 256 directions, the default) or 'closest' (the
    exact distance from one closest-point query).  sign: how `occupancy` tells inside from outside -- 'rays' (the reference's first-hit
    test, the default) or 'winding' (the generalized winding number: any triangle soup); everything after the occupancy is the same."""
    _check_distance(distance)
    _check_sign(sign)
    tri = load_mesh(mesh_fn) if isinstance(mesh_fn, str) else mesh_fn
    tri = torch.as_tensor(np.asarray(tri) if not torch.is_tensor(tri) else tri, dtype=torch.float32).to(device).reshape(-1, 3, 3).contiguous()
    res = int(resolution)
    cast = _caster(tri, accel)
    values, origins = occupancy(tri, res, cast, sign=sign, accel=accel)
    grid = redistancing.redistance(values)
    if refine_surface:
        grid = redistancing.redistance(refine(tri, grid, origins, res, cast=cast, distance=distance, accel=accel))
    return grid


def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='Triangle mesh (obj / ply, inside [-0.5, 0.5]^3) -> SDF grid, written as a .vol.')
    ap.add_argument('mesh')
    ap.add_argument('-o', '--out', required=True, help='the .vol file to write')
    ap.add_argument('--res', type=int, default=128)
    ap.add_argument('--sign', choices=('rays', 'winding'), default='rays',
                    help="rays: first-hit test (watertight meshes); winding: generalized winding number (any triangle soup)")
    ap.add_argument('--distance', choices=('rays', 'closest'), default='rays')
    a = ap.parse_args(argv)
    if a.res < 2:
        ap.error('--res must be at least 2')
    return a


def main(argv=None):
    import util
    a = parse_args(argv)
    grid = create_sdf(a.mesh, a.res, distance=a.distance, sign=a.sign)
    util.write_vol(a.out, grid.cpu())
    print(f'{a.out}: {a.res}^3, sign={a.sign}, distance={a.distance}')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
