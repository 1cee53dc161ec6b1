"""TEST INFRASTRUCTURE ONLY -- what the vertex-colour tests share (tests/test_gpu_mesh_colors.py, tests/test_mesh_colors_host.py): the
fp64 image oracle of a mesh render with a reflectance per triangle corner, and the cases.

The oracle is the direct branch of tests/mesh_render_oracle.py: render with one statement changed: the reflectance of a hit is
(1 - u - v) c0 + u c1 + v c2 of the corner colours of the triangle `primary` located (k, u, v), not a lookup in a volume."""
import math

import numpy as np
import torch

import mesh_oracle as M
import mesh_render_oracle as R
import sdf_oracle as O

VOLUME_SHAPE = (5, 6, 7)                     # (Z, Y, X): three different extents
AFFINE_A = np.array([[0.5, -0.2, 0.1], [0.1, 0.5, -0.3], [-0.25, 0.15, 0.45]])
AFFINE_B = np.array([0.3, 0.35, 0.35])       # c = A p + b stays inside (0, 1) on the unit cube


def corner_reflectance(colors, k, u, v):
    c = np.asarray(colors, np.float64)[k]
    return (1 - u - v)[:, None] * c[:, 0] + u[:, None] * c[:, 1] + v[:, None] * c[:, 2]


def render_colors(tri, normals, colors, cam, W, H, spp, offsets, emitter_u, env=1.0, hide_emitters=False, prim=None):
    """One view of sdf_direct_reparam over a mesh with corner colours (T, 3, 3) -> image (H, W, 3) float64."""
    pr = prim if prim is not None else R.primary(tri, cam, W, H, spp, offsets)
    o, d, t = pr['o'], pr['d'], pr['t']
    N = o.shape[0]
    hit = np.isfinite(t)
    hs = np.nonzero(hit)[0]
    rgb = np.zeros((N, 3))
    if not hide_emitters:
        rgb[~hit] = env
    if hs.size:
        k, u, v = pr['k'][hs], pr['u'][hs], pr['v'][hs]
        nt = torch.as_tensor(R.normals_at(tri, normals, k, u, v))
        p = o[hs] + torch.as_tensor(t[hs])[:, None] * d[hs]
        wdir = O.square_to_uniform_sphere(emitter_u[hs].to(torch.float64))
        so, sd, smaxt = O.spawn_ray_to(p, nt, p + wdir * O.ENV_DIST)
        fs = np.nonzero(((O.dot(nt, sd) > 0) & (O.dot(nt, -d[hs]) > 0)).numpy())[0]
        if fs.size:
            ts, _, _ = M.raycast(tri, so[fs].numpy(), sd[fs].numpy())
            vis = ~(ts < smaxt[fs].numpy())
            cos_o = O.dot(nt[fs], sd[fs]).numpy()
            a = corner_reflectance(colors, k[fs], u[fs], v[fs])
            rgb[hs[fs]] = a * (cos_o / math.pi)[:, None] * (env * 4.0 * math.pi) * vis[:, None]
    uv, _ = cam.sample_direction(o + d, W, H)
    Wb, Hb = W + 2 * O.BORDER, H + 2 * O.BORDER
    vals = torch.cat([torch.as_tensor(rgb), torch.ones(N, 1, dtype=torch.float64)], 1)
    block = O.block_put(torch.zeros(Hb * Wb * 4, dtype=torch.float64), uv, vals, Wb, Hb)
    return O.develop(block, W, H).numpy()


def texel_centres(shape=VOLUME_SHAPE):
    """(Z * Y * X, 3) float64 points (x, y, z) of the texel centres (i + 0.5) / res."""
    rz, ry, rx = shape
    z, y, x = np.meshgrid((np.arange(rz) + 0.5) / rz, (np.arange(ry) + 0.5) / ry, (np.arange(rx) + 0.5) / rx, indexing='ij')
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], -1)


def affine_volume(shape=VOLUME_SHAPE):
    """(Z, Y, X, 3) float32: c = A p + b at the texel centres.  Its trilinear lookup is that affine function inside
    [0.5 / res, 1 - 0.5 / res]^3 (to the rounding of the stored values)."""
    return torch.from_numpy((texel_centres(shape) @ AFFINE_A.T + AFFINE_B).reshape(*shape, 3)).float().contiguous()


def affine_colors(tri):
    """(T, 3, 3) float32 corner colours A p + b of the triangle corners."""
    return (np.asarray(tri, np.float64) @ AFFINE_A.T + AFFINE_B).astype(np.float32)


def sample_points(shape=VOLUME_SHAPE, seed=0):
    """(n, 3) float32: 1000 random points of [-0.1, 1.1]^3 (the clamp), the texel centres, and points on cell faces -- one coordinate
    with p * res - 0.5 an integer, the other two random."""
    rz, ry, rx = shape
    g = torch.Generator().manual_seed(seed)
    rnd = torch.rand(1000, 3, generator=g, dtype=torch.float64) * 1.2 - 0.1
    faces = []
    for axis, res in enumerate((rx, ry, rz)):
        for i in range(res):
            q = torch.rand(8, 3, generator=g, dtype=torch.float64)
            q[:, axis] = (i + 0.5) / res
            faces.append(q)
    return torch.cat([rnd, torch.from_numpy(texel_centres(shape))] + faces).float().contiguous()
