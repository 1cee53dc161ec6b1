"""Seeded test cases shared by the CPU and GPU parity tests."""
import numpy as np
import torch

import sdf_oracle as O


def make_case(name):
    """Returns dict(grid fp64 (Z,Y,X), cam index/total, W, H, spp, offsets fp32 (n,2), grad_image fp32)."""
    cfg = {
        # name: (grid fn, n_cams, cam_idx, W, H, spp, seed)
        'sphere16': (lambda: O.sphere_grid(16), 1, 0, 16, 16, 4, 1),
        'blob32': (lambda: O.blob_grid(32, n=6, seed=1), 3, 1, 24, 24, 8, 2),
        'blob32_spp64': (lambda: O.blob_grid(32, n=6, seed=1), 3, 2, 12, 12, 64, 3),
        'blob48_rect': (lambda: O.blob_grid(48, n=10, seed=3), 12, 5, 32, 20, 4, 4),
        # three 64-sample chunks per pixel (not a power of two: work-list tiles, chunk -> unit arithmetic)
        'blob32_spp192': (lambda: O.blob_grid(32, n=6, seed=1), 3, 2, 6, 6, 192, 5),
        # 2 spp: 8 x 4 pixel-tile waves of the general pass, film window in LDS, ragged tiles at the right / bottom edge
        'blob32_spp2': (lambda: O.blob_grid(32, n=6, seed=1), 3, 2, 21, 13, 2, 6),
        # 3 spp: neither a power of two nor a multiple of 64 -- the general pass in LINEAR lane order, every sample splatted on its own
        'blob32_spp3': (lambda: O.blob_grid(32, n=6, seed=1), 3, 1, 24, 24, 3, 8),
    }[name]
    gridfn, ncam, icam, W, H, spp, seed = cfg
    gen = torch.Generator().manual_seed(seed)
    offsets = torch.rand((W + 4) * (H + 4) * spp, 2, generator=gen, dtype=torch.float32)
    grad_image = torch.randn(H, W, 3, generator=gen, dtype=torch.float32)
    origin = O.regular_camera_origins(ncam)[icam]
    # the oracle's sensor is the one DEFINED by the fp32 record the C-ABI receives (bit-identical inputs on both sides)
    cam = O.Camera(origin).rounded()
    return dict(name=name, grid=gridfn(), ncam=ncam, icam=icam, origin=origin, cam=cam, W=W, H=H, spp=spp,
                offsets=offsets, grad_image=grad_image)


def oracle_forward(case, integrator, reparam=True):
    cam = case['cam']
    return O.render(O.Grid3d(case['grid']), cam, case['W'], case['H'], case['spp'], case['offsets'].double(),
                    integrator, reparam, return_aux=True)


def oracle_backward(case, integrator, reparam=True):
    cam = case['cam']
    return O.render_backward(O.Grid3d(case['grid']), cam, case['W'], case['H'], case['spp'], case['offsets'].double(),
                             case['grad_image'].double(), integrator, reparam)


def direct_inputs(case, ares=(6, 5, 4), seed=11):
    """Extra inputs of sdf_direct_reparam for a case: albedo volume (Z,Y,X,3) fp32 in [0.2, 0.8], per-lane
    emitter samples (n,2) fp32, environment radiance."""
    gen = torch.Generator().manual_seed(seed)
    n = case['offsets'].shape[0]
    albedo = torch.rand(*ares, 3, generator=gen, dtype=torch.float32) * 0.6 + 0.2
    emitter_u = torch.rand(n, 2, generator=gen, dtype=torch.float32)
    return dict(albedo=albedo, emitter_u=emitter_u, env=(1.0, 0.9, 0.8))


def oracle_direct(case, extra, reparam=True, hide_emitters=False, grads=False, p=None):
    """Oracle image of sdf_direct_reparam; with grads=True also (dL/d data, dL/d albedo[, dL/d p]) for
    L = sum(image * grad_image)."""
    cam = case['cam']
    data = case['grid'].clone().requires_grad_(grads)
    alb = extra['albedo'].double().clone().requires_grad_(grads)
    env = torch.tensor(extra['env'], dtype=torch.float64)
    img = O.render(O.Grid3d(data, p), cam, case['W'], case['H'], case['spp'], case['offsets'].double(), O.DIRECT, reparam,
                   albedo=alb, emitter_u=extra['emitter_u'].double(), env=env, hide_emitters=hide_emitters)
    if not grads:
        return img
    (img * case['grad_image'].double()).sum().backward()
    return img.detach(), data.grad, alb.grad


# Ragged shapes (Z, Y, X): x sizes at every residue mod 4 (the row-block copy's x chunks are 4 taps apart), y / z sizes that are not
# multiples of 8 (partial last blocks of the 8^3 / 4^3 / 2^3 proof bounds), a side thinner than one 8^3 block; films whose sides
# leave partial work-list tiles.  name: (shape, W, H, spp, n_cams, views, seed)
RAGGED = {
    'rag_x1': ((37, 30, 45), 45, 31, 64, 6, (0, 2, 4), 41),        # rx % 4 == 1
    'rag_x2': ((26, 41, 34), 33, 47, 64, 6, (1, 4), 42),           # rx % 4 == 2
    'rag_x3': ((51, 19, 23), 45, 31, 64, 6, (0, 3), 43),           # rx % 4 == 3
    'rag_thin': ((10, 6, 39), 41, 29, 64, 6, (1, 3, 5), 44),       # y and z sides under one 8^3 block
}


def ragged_grid(shape, seed, walls=True):
    """Seeded union of spheres sampled on per-axis linspace (voxel sizes differ per axis), rounded to fp32 and returned as fp64.
    walls=True: sphere 0 crosses the +x and +y faces of the unit box, so that the cells of the last x chunk and of the partial blocks
    hold surface; sphere 1 crosses the +x face near z = 0.  walls=False: the same two spheres moved inwards until they stop 0.6 of a
    voxel short of those faces -- the surface still runs through the last cell of each axis, but never meets a wall of the box
    (where it does, the warp field's 1/denom^3 weights of the grazing samples along the crease make the fp32 gradient a heavy-tailed
    draw: tests/test_gpu_ragged.py)."""
    rng = np.random.default_rng(seed)
    lin = [np.linspace(0, 1, n) for n in shape]
    z, y, x = np.meshgrid(*lin, indexing='ij')
    pts = np.stack([x, y, z], -1)
    rz, ry, rx = shape
    z0, y1 = rng.uniform(0.4, 0.6), rng.uniform(0.3, 0.5)
    if walls:
        spheres = [((0.93, 0.9, z0), 0.2), ((0.97, y1, 0.1), 0.14)]
    else:
        spheres = [((0.8 - 0.6 / (rx - 1), 0.8 - 0.6 / (ry - 1), z0), 0.2), ((0.86 - 0.6 / (rx - 1), y1, 0.14 + 0.6 / (rz - 1)), 0.14)]
    spheres += [(tuple(rng.uniform(0.3, 0.7, 3)), rng.uniform(0.1, 0.2)) for _ in range(3)]
    sd = np.full(tuple(shape), 1e9)
    for c, r in spheres:
        sd = np.minimum(sd, np.linalg.norm(pts - np.asarray(c), axis=-1) - r)
    return torch.tensor(sd.astype(np.float32)).double()


def ragged_case(name, spp=None, walls=True):
    """A make_case dict (view 0 of the case) for a ragged grid and film, plus `views`: one such dict per view of the ring (its own
    cam, offsets and grad_image slice; `name` carries the view), and `offsets` / `grad_image` of all views concatenated in view
    order under `offsets_all` / `grad_image_all` -- what one multi-view call of the HIP path takes.  `spp` overrides the case's
    sample count, walls=False moves the surface off the box walls (ragged_grid); the name then carries either (precision.py caches
    by name)."""
    shape, W, H, spp0, ncam, icams, seed = RAGGED[name]
    grid = ragged_grid(shape, seed, walls)
    if not walls:
        name = f'{name}_inner'
    if spp is not None and spp != spp0:
        name, seed = f'{name}_spp{spp}', seed + spp
    spp = spp or spp0
    gen = torch.Generator().manual_seed(seed)
    origins = O.regular_camera_origins(ncam)
    views = []
    for k, icam in enumerate(icams):
        offsets = torch.rand((W + 4) * (H + 4) * spp, 2, generator=gen, dtype=torch.float32)
        grad_image = torch.randn(H, W, 3, generator=gen, dtype=torch.float32)
        views.append(dict(name=f'{name}_v{icam}', grid=grid, ncam=ncam, icam=icam, origin=origins[icam],
                          cam=O.Camera(origins[icam]).rounded(), W=W, H=H, spp=spp, offsets=offsets, grad_image=grad_image))
    case = dict(views[0], name=name, views=views, icams=list(icams))
    case['offsets_all'] = torch.cat([v['offsets'] for v in views])
    case['grad_image_all'] = torch.stack([v['grad_image'] for v in views])
    return case
