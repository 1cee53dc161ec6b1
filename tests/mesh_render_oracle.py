"""TEST INFRASTRUCTURE ONLY -- the fp64 image oracle of a mesh render (dsdf.mesh_render), composed from existing parts: the
sensor, lane order, film and shading statements of oracle/sdf_oracle.py and the ray caster of oracle/mesh_oracle.py.  The per-sample
value is the primal statement of the three integrators with the intersection routine swapped (no warp, det = 1):
    silhouette      [hit]
    simple shading  max(n . l, 0)
    direct          sdf_direct_reparam.py:29-75, use_mis = False: escaping rays see the environment unless hide_emitters; emitter
                    direction square_to_uniform_sphere(emitter_u); shadow ray through spawn_ray_to, an any-hit query up to maxt;
                    both cosines positive; albedo(p) cos_o / pi * env * 4 pi when unoccluded
with n the normalised barycentric interpolation of the vertex normals, or the geometric normal (p1 - p0) x (p2 - p0)."""
import math

import numpy as np
import torch

import mesh_oracle as M
import sdf_oracle as O


def locate(tri, o, d, t_min=0.0, block=2048):
    """The triangle M.raycast hits and where: (t, k, u, v) per ray, k = -1 on a miss.  The same statements as M.raycast, so the
    distances are its distances bit for bit (asserted by the callers that use both)."""
    tri = np.asarray(tri, np.float64); o = np.asarray(o, np.float64); d = np.asarray(d, np.float64)
    p0 = tri[:, 0]; e1 = tri[:, 1] - p0; e2 = tri[:, 2] - p0
    n = o.shape[0]
    t_best = np.full(n, np.inf); kk = np.full(n, -1, np.int64); uu = np.zeros(n); vv = np.zeros(n)
    for s in range(0, n, block):
        oo = o[s:s + block, None, :]; dd = d[s:s + block, None, :]
        pv = np.cross(dd, e2[None])
        det = (e1[None] * pv).sum(-1)
        safe = np.where(det != 0, det, 1.0)
        tv = oo - p0[None]
        u = (tv * pv).sum(-1) / safe
        qv = np.cross(tv, e1[None])
        v = (dd * qv).sum(-1) / safe
        t = (e2[None] * qv).sum(-1) / safe
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > t_min)
        tt = np.where(ok, t, np.inf)
        k = tt.argmin(1)
        r = np.arange(tt.shape[0])
        t_best[s:s + block] = tt[r, k]
        kk[s:s + block] = np.where(np.isfinite(tt[r, k]), k, -1)
        uu[s:s + block] = u[r, k]; vv[s:s + block] = v[r, k]
    return t_best, kk, uu, vv


def normals_at(tri, normals, k, u, v):
    tri = np.asarray(tri, np.float64)
    if normals is None:
        n = np.cross(tri[k, 1] - tri[k, 0], tri[k, 2] - tri[k, 0])
    else:
        nn = np.asarray(normals, np.float64)[k]
        n = (1 - u - v)[:, None] * nn[:, 0] + u[:, None] * nn[:, 1] + v[:, None] * nn[:, 2]
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def primary(tri, cam, W, H, spp, offsets):
    """Camera rays of one view in lane order and their closest hits (shared by the integrators of a case)."""
    pos = O.lane_positions(W, H, spp, offsets.to(torch.float64))
    o, d, _ = cam.sample_ray(pos, W, H)
    t, _, margin = M.raycast(tri, o.numpy(), d.numpy())
    n = t.shape[0]
    k = np.full(n, -1, np.int64); u = np.zeros(n); v = np.zeros(n)
    hs = np.nonzero(np.isfinite(t))[0]                                       # (the triangle and barycentrics of the rays that hit only)
    if hs.size:
        t2, k[hs], u[hs], v[hs] = locate(tri, o.numpy()[hs], d.numpy()[hs])
        assert np.array_equal(t[hs], t2)
    return dict(o=o, d=d, t=t, k=k, u=u, v=v, margin=margin)


def render(tri, normals, cam, W, H, spp, offsets, integrator, albedo=None, emitter_u=None, env=1.0, hide_emitters=False, prim=None,
           occlusion=True):
    """One view -> image (H, W, 3) float64.  offsets: (Wb * Hb * spp, 2) in [0, 1); prim: primary(...) of the same view, if at hand;
    occlusion=False leaves the shadow query out (what an image WITHOUT shadows would be: the tests use it to show that theirs has some)."""
    pr = prim if prim is not None else primary(tri, cam, W, H, spp, offsets)
    o, d, t = pr['o'], pr['d'], pr['t']
    N = o.shape[0]
    hit = np.isfinite(t)
    hs = np.nonzero(hit)[0]
    rgb = np.zeros((N, 3))
    n = normals_at(tri, normals, pr['k'][hs], pr['u'][hs], pr['v'][hs]) if hs.size else np.zeros((0, 3))
    if integrator == O.SILHOUETTE:
        rgb[hs] = 1.0
    elif integrator == O.SIMPLE_SHADING:
        light = np.ones(3) / math.sqrt(3.0)
        rgb[hs] = np.clip(n @ light, 0.0, None)[:, None]
    else:
        if not hide_emitters:
            rgb[~hit] = env
        if hs.size:
            p = o[hs] + torch.as_tensor(t[hs])[:, None] * d[hs]
            nt = torch.as_tensor(n)
            wdir = O.square_to_uniform_sphere(emitter_u[hs].to(torch.float64))
            so, sd, smaxt = O.spawn_ray_to(p, nt, p + wdir * O.ENV_DIST)
            front = ((O.dot(nt, sd) > 0) & (O.dot(nt, -d[hs]) > 0)).numpy()
            fs = np.nonzero(front)[0]
            if fs.size:
                ts, _, _ = M.raycast(tri, so[fs].numpy(), sd[fs].numpy())
                vis = ~(ts < smaxt[fs].numpy()) if occlusion else np.ones(fs.size, bool)
                cos_o = O.dot(nt[fs], sd[fs]).numpy()
                a = O.eval_trilinear(albedo.to(torch.float64), p[fs]).numpy()
                rgb[hs[fs]] = a * (cos_o / math.pi)[:, None] * (env * 4.0 * math.pi) * vis[:, None]
    uv, _ = cam.sample_direction(o + d, W, H)
    Wb, Hb = W + 2 * O.BORDER, H + 2 * O.BORDER
    vals = torch.cat([torch.as_tensor(rgb), torch.ones(N, 1, dtype=torch.float64)], 1)
    block = O.block_put(torch.zeros(Hb * Wb * 4, dtype=torch.float64), uv, vals, Wb, Hb)
    return O.develop(block, W, H).numpy()
