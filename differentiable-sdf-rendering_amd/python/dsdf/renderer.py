"""Host-side operators over the C-ABI (include/dsdf.h) on torch HIP tensors.

torch is used for device memory, streams and autograd plumbing only; every
kernel on the path is in libdsdf.so.  `render()` plays the role of `mi.render`
with the reference's `_RenderOp` semantics (python/shape_opt.py:78-80): the
primal image comes from an (seed, spp) render without gradients, the backward
from an independent (seed_grad, spp_grad) re-render
(python/integrators/reparam.py:187-190).
"""
import contextlib
import ctypes as C
import math
import os

import torch

from . import _lib
from ._lib import (DSDF_DIRECT, DSDF_NO_FINE_EMPTY, DSDF_NO_HIT_PROOF, DSDF_NO_VALUE_BOUND, DSDF_NO_SKIP, DSDF_REPARAM, DSDF_SILHOUETTE, DSDF_SIMPLE_SHADING, DsdfCamera,
                   DsdfShading)

INTEGRATORS = {'sdf_silhouette_reparam': DSDF_SILHOUETTE, 'sdf_simple_shading_reparam': DSDF_SIMPLE_SHADING,
               'sdf_direct_reparam': DSDF_DIRECT,
               DSDF_SILHOUETTE: DSDF_SILHOUETTE, DSDF_SIMPLE_SHADING: DSDF_SIMPLE_SHADING, DSDF_DIRECT: DSDF_DIRECT}

STAT_NAMES = ('lanes', 'bbox_lanes', 'steps', 'hits', 'refine_steps', 'warp_active', 'queue_len', 'wave_steps',
              'tail_steps', 'tail_wave_steps', 'tail_rays')
STAT_SLOTS = 16          # include/dsdf.h: DSDF_STAT_SLOTS

_workspaces = {}


def _proof_flags(empty_space_skip):
    """True: both per-pixel proofs (csrc/dsdf_proof.h); 'empty-only': without the hit proof of the silhouette primal; 'coarse-empty':
    without the second stage of the empty-space proof on the full-resolution window minima, and the third with it; 'window-empty':
    without the third stage only, the spline value on the centre ray -+ a gradient bound (both A/B and tests); False: none."""
    if empty_space_skip == 'empty-only':
        return DSDF_NO_HIT_PROOF
    if empty_space_skip == 'coarse-empty':
        return DSDF_NO_FINE_EMPTY
    if empty_space_skip == 'window-empty':
        return DSDF_NO_VALUE_BOUND
    return 0 if empty_space_skip else DSDF_NO_SKIP

# Views traced by one kernel launch (bounded by the workspace: the backward queue of a GRADIENT pass holds 40 B per
# sample and view -- 16 views x 512^2 x 64 spp = 11 GB, cheap in 288 GB of HBM; a primal render carries no queue).
MAX_VIEWS_PER_LAUNCH = 16


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _floats(a):
    return (C.c_float * len(a))(*[float(v) for v in a])


def _as_list(sensors):
    return list(sensors) if isinstance(sensors, (list, tuple)) else [sensors]


def _require_dev(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.DsdfError(f"{name} must be a torch tensor on the HIP device (got {type(t).__name__}"
                             f"{'' if not isinstance(t, torch.Tensor) else ' on ' + str(t.device)}); no CPU path exists")
    if t.dtype != dtype:
        raise _lib.DsdfError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


def _workspace(device, nbytes, min_bytes=None):
    """Per-device scratch buffer, grown on demand.  When the device cannot provide `nbytes` (a gradient-pass workspace for
    16 views x 512^2 x 64 spp is 11 GB) the request is halved down to `min_bytes` (one view per launch): the C side batches
    as many views per launch as the workspace it is given allows."""
    ws = _workspaces.get(device)
    if ws is not None and ws.numel() >= nbytes:
        return ws
    _workspaces.pop(device, None)
    del ws
    want = int(nbytes)
    while True:
        try:
            ws = torch.empty(want, dtype=torch.uint8, device=device)
            break
        except torch.OutOfMemoryError:
            if min_bytes is None or want <= int(min_bytes):
                raise
            torch.cuda.empty_cache()
            want = max(int(min_bytes), want // 2)
    _workspaces[device] = ws
    return ws


def release_workspaces():
    """Frees the cached scratch buffers (they are kept between calls otherwise)."""
    _workspaces.clear()
    _sweep_workspaces.clear()


class SdfGrid:
    """Device-side SDF grid: `sdf.data` (Z,Y,X[,1]) plus the library's padded copy.
    Mirrors what `Grid3d.__init__/update/parameters_changed` do with the Dr.Jit
    texture (python/shapes.py:378-403, 473-479)."""

    def __init__(self, data, params=None, to_world=None):
        self.params = params if params is not None else _lib.default_params()
        self.padded = None
        self.transform = None
        self.version = 0                                   # counts update() calls: a gradient sweep remembers which grid it traced
        if to_world is not None:
            self.set_to_world(to_world)
        self.update(data)

    def set_to_world(self, to_world):
        """A GENERAL `to_world` (4x4, affine: any rotation, scale) for this grid (python/shapes.py:378-403): its calls go to the
        world-space build of the library (lib/variants/libdsdf_xf.so, include/dsdf.h: dsdf_set_grid_transform) with
        to_local = to_world^-1 and the world AABB of the transformed cube; rays, sensors and `sdf.p` stay in world space."""
        import numpy as np
        tw = np.asarray(to_world, np.float64).reshape(4, 4)
        if not np.allclose(tw[3], [0, 0, 0, 1], atol=1e-12):
            raise _lib.DsdfError("to_world must be affine")
        inv = np.linalg.inv(tw)
        corners = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
        w = corners @ tw[:3, :3].T + tw[:3, 3]
        self.transform = (_floats(inv[:3, :].reshape(-1)), _floats(w.min(0)), _floats(w.max(0)))
        self.to_world = tw
        return self

    _IDENTITY = None

    def lib(self, extended=False):
        """The library this grid's calls go to; for a grid with a general transform the world-space build, with the transform
        (re-)applied (it is state of that library instance, include/dsdf.h: dsdf_set_grid_transform).  extended=True routes THIS
        call of a transform-free grid to that build with the identity -- `use_mis` with the principled BSDF lives there --
        without changing the grid: its other calls keep the default library and its per-pixel proofs."""
        if self.transform is None and not extended:
            return _lib.load()
        tf = self.transform
        if tf is None:
            if SdfGrid._IDENTITY is None:
                SdfGrid._IDENTITY = (_floats([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]), _floats([0, 0, 0]), _floats([1, 1, 1]))
            tf = SdfGrid._IDENTITY
        lib = _lib.load_xf()
        with torch.cuda.device(self.device):
            _lib.check(lib.dsdf_set_grid_transform(tf[0], tf[1], tf[2], _stream()), lib)
        return lib

    def update(self, data):
        lib = _lib.load()                                  # (dsdf_padded_size / dsdf_pad_grid know nothing of a transform: any build serves)
        if data.dim() == 4:
            if data.shape[3] != 1:
                raise _lib.DsdfError("sdf.data must have one channel")
            data = data[..., 0]
        if data.dim() != 3:
            raise _lib.DsdfError(f"sdf.data must be (Z,Y,X) or (Z,Y,X,1), got {tuple(data.shape)}")
        data = _require_dev(data.detach(), 'sdf.data')
        self.rz, self.ry, self.rx = (int(s) for s in data.shape)
        n = lib.dsdf_padded_size(self.rx, self.ry, self.rz)
        if self.padded is None or self.padded.numel() != n or self.padded.device != data.device:
            self.padded = torch.empty(n, dtype=torch.float32, device=data.device)
        with torch.cuda.device(data.device):
            _lib.check(lib.dsdf_pad_grid(_ptr(data), self.rx, self.ry, self.rz, _ptr(self.padded), _stream()))
        self.device = data.device
        self.version += 1
        # what the padded copy was built from: the tensor OBJECT (held, so its storage cannot be recycled for another tensor
        # while it is the key) and its in-place version
        self._src = (data, data._version)
        return self

    def in_sync_with(self, data):
        """True when the padded copy was built from exactly this tensor state (storage and in-place version)."""
        src = getattr(self, '_src', None)
        if src is None:
            return False
        t, ver = src
        d = data.detach()
        # `t` is held, so its storage is alive: an equal address is the same memory, not a recycled block
        return t.data_ptr() == d.data_ptr() and t.numel() == d.numel() and d._version == ver

    def set_translation(self, p):
        """`sdf.p` (python/shapes.py:389, 412): lookups happen at x - p.  A tensor is ALWAYS read back (3 floats): its
        address and in-place version do not identify its contents -- a temporary (`p0 + eps * e` in a finite-difference
        loop) is freed and re-allocated at the same address with version 0."""
        if isinstance(p, torch.Tensor):
            # ... but the SAME tensor object at the same in-place version holds what was read last time: no second
            # device-to-host read-back (a blocking sync per call when sdf.p lives on the GPU).  The object is
            # held, so its storage cannot be recycled for another tensor meanwhile.
            # (only for a tensor whose in-place version is tracked: inference-mode tensors have none, and writes through `.data`
            # / `set_()` do not bump it -- a leaf that is edited that way must be passed as a list, or after any in-place op)
            try:
                ver = p._version
            except (RuntimeError, AttributeError):
                ver = None
            src = getattr(self, '_p_src', None)
            if ver is not None and src is not None and src[0] is p and src[1] == ver:
                return self
            vals = p.detach().cpu().tolist()
            self._p_src = (p, ver) if ver is not None else None
        else:
            vals = p
            self._p_src = None
        px, py, pz = (float(v) for v in vals)
        self.params.sdf_p[0], self.params.sdf_p[1], self.params.sdf_p[2] = px, py, pz
        return self

    @property
    def shape(self):
        return (self.rz, self.ry, self.rx)


def _needs_extended(shading):
    """`use_mis` with the principled BSDF (Principled::sample / ::pdf) exists in the extended build of the library only."""
    return shading is not None and shading.roughness is not None and shading.use_mis


class Shading:
    """Scene-side inputs of `sdf_direct_reparam` (python/integrators/sdf_direct_reparam.py): the diffuse
    BSDF's reflectance volume `albedo` (Z,Y,X,3) -- 'main-bsdf.reflectance.volume.data',
    python/opt_configs.py:286 -- and a constant environment emitter (include/dsdf.h: dsdf_shading).
    use_mis (reparam.py:17): emitter sampling + BSDF sampling with the power heuristic; detach_indirect_si /
    decouple_reparam: the integrator properties of the same names (sdf_direct_reparam.py:13-14, 44-47).
    roughness (Z,Y,X,1): switches the BSDF to `principled` at the plugin defaults -- `albedo` is then its base_color volume and
    `roughness` 'main-bsdf.roughness.volume.data' (python/opt_configs.py:288-299); a gradient call accumulates dL/d(roughness)
    into `grad_roughness` (a tensor shaped like roughness, set on the object) next to grad_albedo.
    albedo=None is legal for dsdf.mesh_render of a MeshBvh that carries corner colours (they are the reflectance then); every other
    entry point refuses it."""

    def __init__(self, albedo, env_radiance=(1.0, 1.0, 1.0), hide_emitters=False, use_mis=False, detach_indirect_si=False,
                 decouple_reparam=False, roughness=None):
        self.albedo = albedo
        self.roughness = roughness
        self.grad_roughness = None
        self.env_radiance = (float(env_radiance),) * 3 if isinstance(env_radiance, (int, float)) else tuple(env_radiance)
        self.hide_emitters = bool(hide_emitters)
        self.use_mis = bool(use_mis)
        self.detach_indirect_si, self.decouple_reparam = bool(detach_indirect_si), bool(decouple_reparam)

    def with_albedo(self, albedo):
        return Shading(albedo, self.env_radiance, self.hide_emitters, self.use_mis, self.detach_indirect_si, self.decouple_reparam,
                       self.roughness)

    def to_struct(self, n_views, n_lanes, emitter_samples=None, grad_albedo=None, bsdf_samples=None, need_albedo=True):
        st = DsdfShading()
        keep = []
        if self.albedo is None:
            if need_albedo or grad_albedo is not None:
                raise _lib.DsdfError("Shading(albedo=None) serves dsdf.mesh_render of a MeshBvh with corner colours only: this call reads "
                                     "the reflectance volume, pass albedo (Z,Y,X,3)")
        else:
            a = self.albedo.detach()
            if a.dim() != 4 or a.shape[3] != 3:
                raise _lib.DsdfError(f"albedo must be (Z,Y,X,3), got {tuple(a.shape)}")
            a = _require_dev(a, 'albedo')
            st.albedo = a.data_ptr()
            st.az, st.ay, st.ax = (int(v) for v in a.shape[:3])
            keep.append(a)
        st.env_radiance[0], st.env_radiance[1], st.env_radiance[2] = self.env_radiance
        st.hide_emitters = int(self.hide_emitters)
        st.use_mis = int(self.use_mis)
        st.variant = 1 if self.detach_indirect_si else (2 if self.decouple_reparam else 0)   # (the reference tests them in this order)
        for name, t in (('emitter_samples', emitter_samples), ('bsdf_samples', bsdf_samples)):
            if t is None:
                continue
            t = _require_dev(t, name)
            if t.numel() != n_views * n_lanes * 2:
                raise _lib.DsdfError(f"{name} must hold n_views*(W+4)*(H+4)*spp*2 = {n_views * n_lanes * 2} floats")
            setattr(st, name, t.data_ptr())
            keep.append(t)
        if grad_albedo is not None:
            if tuple(grad_albedo.shape) != tuple(a.shape) or not grad_albedo.is_contiguous():
                raise _lib.DsdfError("grad_albedo must be a contiguous tensor shaped like albedo")
            _require_dev(grad_albedo, 'grad_albedo')
            st.grad_albedo = grad_albedo.data_ptr()
        if self.roughness is not None:
            r = self.roughness.detach()
            if r.dim() == 3:
                r = r[..., None]
            if r.dim() != 4 or r.shape[3] != 1:
                raise _lib.DsdfError(f"roughness must be (Z,Y,X,1), got {tuple(self.roughness.shape)}")
            r = _require_dev(r, 'roughness')
            st.bsdf = 1
            st.roughness = r.data_ptr()
            st.raz, st.ray, st.rax = (int(v) for v in r.shape[:3])
            keep.append(r)
            gr = self.grad_roughness
            if grad_albedo is not None and gr is not None:
                if gr.numel() != r.numel() or not gr.is_contiguous():
                    raise _lib.DsdfError("grad_roughness must be a contiguous tensor shaped like roughness")
                _require_dev(gr, 'grad_roughness')
                st.grad_roughness = gr.data_ptr()
                keep.append(gr)
        lobe = getattr(self, 'lobe_samples', None)       # explicit next_1d() of bsdf.sample (principled + use_mis; tests): (n_views, lanes)
        if lobe is not None and self.roughness is not None and self.use_mis:
            lobe = _require_dev(lobe, 'lobe_samples')
            if lobe.numel() != n_views * n_lanes:
                raise _lib.DsdfError(f"lobe_samples must hold n_views*(W+4)*(H+4)*spp = {n_views * n_lanes} floats")
            st.bsdf_lobe_samples = lobe.data_ptr()
            keep.append(lobe)
        return st, keep


def eval_cubic(grid, points, order=2):
    """A1. points (n,3) -> v (n,), g (n,3), H (n,6: xx,yy,zz,xy,xz,yz)."""
    lib = grid.lib()
    points = _require_dev(points, 'points')
    n = points.shape[0]
    dev = points.device
    v = torch.empty(n, dtype=torch.float32, device=dev)
    g = torch.empty(n, 3, dtype=torch.float32, device=dev) if order >= 1 else None
    H = torch.empty(n, 6, dtype=torch.float32, device=dev) if order >= 2 else None
    with torch.cuda.device(dev):
        _lib.check(lib.dsdf_eval_cubic(_ptr(grid.padded), grid.rx, grid.ry, grid.rz, C.byref(grid.params), _ptr(points),
                                       n, order, _ptr(v), _ptr(g), _ptr(H), _stream()))
    return v, g, H


def trace(grid, rays_o, rays_d, maxt, differentiable=True):
    """A2/A4/A5: per-ray sphere tracing. Returns dict of per-ray outputs."""
    lib = grid.lib()
    rays_o = _require_dev(rays_o, 'rays_o'); rays_d = _require_dev(rays_d, 'rays_d'); maxt = _require_dev(maxt, 'maxt')
    n = rays_o.shape[0]
    dev = rays_o.device
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    out = dict(its_t=f(n), warp_t=f(n), warp_t_d=f(n, 3), warp_weight=f(n), warp_weight_d=f(n, 3),
               steps=torch.empty(n, dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        _lib.check(lib.dsdf_trace(_ptr(grid.padded), grid.rx, grid.ry, grid.rz, C.byref(grid.params), _ptr(rays_o),
                                  _ptr(rays_d), _ptr(maxt), n, int(bool(differentiable)), _ptr(out['its_t']),
                                  _ptr(out['warp_t']), _ptr(out['warp_t_d']), _ptr(out['warp_weight']),
                                  _ptr(out['warp_weight_d']), _ptr(out['steps']), _stream()))
    return out


def warp_eval(grid, rays_o, rays_d, trace_out):
    """A9 per ray: `WarpField2D.eval` (python/warp.py:47-96) as its linearisation in (v, g) at x = o + warp_t d.
    trace_out: the dict returned by trace(..., differentiable=True).  Returns dict(active, cdir, a, b, div)."""
    lib = grid.lib()
    rays_o = _require_dev(rays_o, 'rays_o'); rays_d = _require_dev(rays_d, 'rays_d')
    n = rays_o.shape[0]
    dev = rays_o.device
    t = {k: _require_dev(trace_out[k], k) for k in ('warp_t', 'warp_t_d', 'warp_weight', 'warp_weight_d')}
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    out = dict(active=torch.empty(n, dtype=torch.int32, device=dev), cdir=f(n, 3), a=f(n), b=f(n, 3), div=f(n))
    with torch.cuda.device(dev):
        _lib.check(lib.dsdf_warp_eval(_ptr(grid.padded), grid.rx, grid.ry, grid.rz, C.byref(grid.params), _ptr(rays_o), _ptr(rays_d),
                                      n, _ptr(t['warp_t']), _ptr(t['warp_t_d']), _ptr(t['warp_weight']), _ptr(t['warp_weight_d']),
                                      _ptr(out['active']), _ptr(out['cdir']), _ptr(out['a']), _ptr(out['b']), _ptr(out['div']), _stream()))
    return out


def surface_interaction(grid, rays_o, rays_d, t):
    """A6 per ray: `SDFBase.compute_surface_interaction` (python/shapes.py:347-366) -> dict(p, n, grad, t_coef)."""
    lib = grid.lib()
    rays_o = _require_dev(rays_o, 'rays_o'); rays_d = _require_dev(rays_d, 'rays_d'); t = _require_dev(t, 't')
    n = rays_o.shape[0]
    dev = rays_o.device
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    out = dict(p=f(n, 3), n=f(n, 3), grad=f(n, 3), t_coef=f(n))
    with torch.cuda.device(dev):
        _lib.check(lib.dsdf_surface_interaction(_ptr(grid.padded), grid.rx, grid.ry, grid.rz, C.byref(grid.params), _ptr(rays_o),
                                                _ptr(rays_d), _ptr(t), n, _ptr(out['p']), _ptr(out['n']), _ptr(out['grad']),
                                                _ptr(out['t_coef']), _stream()))
    return out


def _views(sensors):
    sensors = _as_list(sensors)
    W, H = sensors[0].film_size()
    for s in sensors:
        if s.film_size() != (W, H):
            raise _lib.DsdfError("all sensors of one call must share the film size")
    cams = (DsdfCamera * len(sensors))(*[s.to_struct() for s in sensors])
    return sensors, cams, W, H


def _sampler_args(n_views, seeds, offsets, n_lanes):
    """(offsets, seeds) of a render call.  Explicit offsets replace the FILM sample of every lane; seeds given next to them still
    seed the later dimensions of the lane's stream (emitter / BSDF samples of sdf_direct_reparam: include/dsdf.h)."""
    cseeds = None
    if seeds is not None:
        seeds = [seeds] * n_views if isinstance(seeds, int) else list(seeds)
        if len(seeds) != n_views:
            raise _lib.DsdfError("one seed per view is required")
        cseeds = (C.c_uint32 * n_views)(*[int(s) & 0xffffffff for s in seeds])
    if offsets is not None:
        offsets = _require_dev(offsets, 'offsets')
        if offsets.numel() != n_views * n_lanes * 2:
            raise _lib.DsdfError(f"offsets must hold n_views*(W+4)*(H+4)*spp*2 = {n_views * n_lanes * 2} floats, "
                                 f"got {offsets.numel()}")
        return offsets, cseeds
    if cseeds is None:
        raise _lib.DsdfError("either seeds or offsets is required")
    return None, cseeds


class _Call:
    """One render call as the library takes it: what the render entry points of include/dsdf.h share -- the library the grid's
    calls go to, views, sampler, integrator, flags, shading -- checked and converted once."""

    def __init__(self, grid, sensors, spp, seeds=None, offsets=None, integrator=DSDF_SILHOUETTE, reparam=True, empty_space_skip=True,
                 shading=None, emitter_samples=None, bsdf_samples=None, grad_albedo=None):
        self.grid, self.params = grid, grid.params
        self.extended = _needs_extended(shading)
        self.lib = grid.lib(self.extended)
        self.sensors, self.cams, self.W, self.H = _views(sensors)
        self.nv, self.spp = len(self.sensors), int(spp)
        self.n_lanes = (self.W + 4) * (self.H + 4) * self.spp
        self.offsets, self.cseeds = _sampler_args(self.nv, seeds, offsets, self.n_lanes)
        self.integrator = INTEGRATORS[integrator]
        self.flags = (DSDF_REPARAM if reparam else 0) | _proof_flags(empty_space_skip)
        self.sh = self._keep = None
        if self.integrator == DSDF_DIRECT:
            if shading is None:
                raise _lib.DsdfError("sdf_direct_reparam needs shading=dsdf.Shading(albedo, ...)")
            st, keep = shading.to_struct(self.nv, self.n_lanes, emitter_samples, grad_albedo, bsdf_samples)
            self.sh, self._keep = C.byref(st), (st, keep)      # (_keep: the struct and the tensors it points to, alive with this object)

    def args(self):
        """The leading arguments of every render entry point."""
        g = self.grid
        return (_ptr(g.padded), g.rx, g.ry, g.rz, C.byref(self.params), self.cams, self.nv, self.W, self.H, self.spp,
                _ptr(self.offsets), self.cseeds, self.integrator, self.flags, self.sh)

    def workspace(self, diff):
        """The device's cached scratch buffer, sized for the views of one launch of a gradient pass (diff) or a primal one."""
        size = self.lib.dsdf_render_workspace_size if diff else self.lib.dsdf_forward_workspace_size
        extra = 0
        if not diff and self.integrator == DSDF_DIRECT:
            # room for the cell table of the shadow rays behind the workspace proper (include/dsdf.h: dsdf_cell_table_size)
            extra = int(self.lib.dsdf_cell_table_size(self.grid.rx, self.grid.ry, self.grid.rz)) + 256
        return _workspace(self.grid.device, size(self.W, self.H, self.spp, min(self.nv, MAX_VIEWS_PER_LAUNCH), self.integrator) + extra,
                          size(self.W, self.H, self.spp, 1, self.integrator))

    def image(self, wanted=True):
        return torch.empty(self.nv, self.H, self.W, 3, dtype=torch.float32, device=self.grid.device) if wanted else None

    def run(self, entry, *tail):
        """lib.<entry>(the shared arguments, *tail, stream) on the grid's device."""
        with torch.cuda.device(self.grid.device):
            _lib.check(getattr(self.lib, entry)(*self.args(), *tail, _stream()))


def sampler_offsets(sensors, spp, seeds, mirror=False, device=None):
    """`sampler.next_2d()` of the built-in `independent` sampler for every lane of every view -> (n_views, (W+4)(H+4)spp, 2); mirror:
    1 - r, the film offsets of the antithetic pair (python/integrators/reparam.py:167-178; dsdf_sampler_2d)."""
    lib = _lib.load()
    sensors, _, W, H = _views(sensors)
    nv = len(sensors)
    n_lanes = (W + 4) * (H + 4) * int(spp)
    _, cseeds = _sampler_args(nv, seeds, None, n_lanes)
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    out = torch.empty(nv, n_lanes, 2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.dsdf_sampler_2d(cseeds, nv, W, H, int(spp), int(bool(mirror)), _ptr(out), _stream()))
    return out


def render_forward(grid, sensors, spp, seeds=None, offsets=None, integrator=DSDF_SILHOUETTE, reparam=True, stats=None,
                   empty_space_skip=True, shading=None, emitter_samples=None, bsdf_samples=None):
    """`ReparamIntegrator.render` for a batch of views -> (n_views, H, W, 3).  `shading` (dsdf.Shading) and the
    optional per-lane `emitter_samples` belong to sdf_direct_reparam."""
    c = _Call(grid, sensors, spp, seeds, offsets, integrator, reparam, empty_space_skip, shading, emitter_samples, bsdf_samples)
    img = c.image()
    ws = c.workspace(False)
    c.run('dsdf_render_forward', _ptr(img), _ptr(ws), ws.numel(), _ptr(stats))
    return img


AOV_NAMES = ['sdf_value', 'warp_t', 'vx', 'vy', 'div', 'i', 'weight_sum', 'weight', 'warp_t_dx', 'warp_t_dy', 'warp_t_dz']   # reparam.py:265


def render_aovs(grid, sensors, spp, seeds=None, offsets=None):
    """The debug channels of `use_aovs` + `WarpField2D.return_aovs` (python/integrators/reparam.py:160-165, 263-267) for a batch of
    views -> (n_views, H, W, 11) in the order of AOV_NAMES.  The reference writes two of them, the loop state of the primary
    ray's differentiable trace (`i`, `weight_sum`: python/shapes.py:240-242; dsdf_render_aovs); the other nine are zero there too."""
    c = _Call(grid, sensors, spp, seeds, offsets)
    lib, nv, W, H, dev = c.lib, c.nv, c.W, c.H, grid.device
    two = torch.empty(nv, H, W, 2, dtype=torch.float32, device=dev)
    ws = _workspace(dev, lib.dsdf_aov_workspace_size(W, H, min(nv, MAX_VIEWS_PER_LAUNCH)), lib.dsdf_aov_workspace_size(W, H, 1))
    with torch.cuda.device(dev):
        # (the AOV pass takes the call up to its sampler: no integrator, flags or shading)
        _lib.check(lib.dsdf_render_aovs(*c.args()[:12], _ptr(two), _ptr(ws), ws.numel(), _stream()))
    out = torch.zeros(nv, H, W, len(AOV_NAMES), dtype=torch.float32, device=dev)
    out[..., AOV_NAMES.index('i')] = two[..., 0]
    out[..., AOV_NAMES.index('weight_sum')] = two[..., 1]
    return out


def render_backward(grid, sensors, spp, grad_image, grad_grid=None, seeds=None, offsets=None,
                    integrator=DSDF_SILHOUETTE, reparam=True, stats=None, return_image=False, empty_space_skip=True,
                    grad_p=None, shading=None, emitter_samples=None, grad_albedo=None, bsdf_samples=None):
    """`ReparamIntegrator.render_backward`: accumulates dL/dsdf into grad_grid (Z,Y,X) and, if given,
    dL/d(sdf.p) into grad_p (3 floats on the device; `sdf.p`, python/shapes.py:471) and, for
    sdf_direct_reparam, dL/d(albedo) into grad_albedo (shaped like shading.albedo)."""
    c = _Call(grid, sensors, spp, seeds, offsets, integrator, reparam, empty_space_skip, shading, emitter_samples, bsdf_samples, grad_albedo)
    nv, W, H, dev = c.nv, c.W, c.H, grid.device
    grad_image = _require_dev(grad_image, 'grad_image')
    if grad_image.numel() != nv * H * W * 3:
        raise _lib.DsdfError(f"grad_image must be (n_views,H,W,3) = {(nv, H, W, 3)}, got {tuple(grad_image.shape)}")
    if grad_grid is None:
        grad_grid = torch.zeros(grid.rz, grid.ry, grid.rx, dtype=torch.float32, device=dev)
    else:
        if tuple(grad_grid.shape[:3]) != grid.shape or not grad_grid.is_contiguous():
            raise _lib.DsdfError("grad_grid must be a contiguous (Z,Y,X) tensor matching the grid")
        _require_dev(grad_grid, 'grad_grid')
    if grad_p is not None:
        if grad_p.numel() != 3 or grad_p.dtype != torch.float32 or not grad_p.is_contiguous():
            raise _lib.DsdfError("grad_p must be a contiguous float32 tensor of 3 elements")
        _require_dev(grad_p, 'grad_p')
    img = c.image(return_image)
    ws = c.workspace(True)
    c.run('dsdf_render_backward', _ptr(grad_image), _ptr(grad_grid), _ptr(grad_p), _ptr(img), _ptr(ws), ws.numel(), _ptr(stats))
    return (grad_grid, img) if return_image else grad_grid


def render_forward_grad(grid, sensors, spp, tangent_data=None, tangent_p=None, seeds=None, offsets=None,
                        integrator=DSDF_SILHOUETTE, reparam=True, return_image=False, empty_space_skip=True, shading=None,
                        emitter_samples=None, bsdf_samples=None):
    """`ReparamIntegrator.render_forward` (python/integrators/reparam.py:192-196): forward-mode gradient image(s)
    (n_views,H,W,3) for a tangent on sdf.data (tensor shaped like the grid) and / or on sdf.p (3 floats)."""
    c = _Call(grid, sensors, spp, seeds, offsets, integrator, reparam, empty_space_skip, shading, emitter_samples, bsdf_samples)
    tpad = None
    if tangent_data is not None:
        t = tangent_data[..., 0] if tangent_data.dim() == 4 else tangent_data
        if tuple(t.shape) != grid.shape:
            raise _lib.DsdfError(f"tangent_data must match the grid {grid.shape}, got {tuple(t.shape)}")
        tpad = SdfGrid(t, grid.params).padded
    tp = None
    if tangent_p is not None:
        vals = tangent_p.detach().cpu().tolist() if isinstance(tangent_p, torch.Tensor) else list(tangent_p)
        tp = (C.c_float * 3)(*[float(v) for v in vals])
    if tpad is None and tp is None:
        raise _lib.DsdfError("render_forward_grad needs tangent_data and / or tangent_p")
    out, img = c.image(), c.image(return_image)
    ws = c.workspace(True)
    c.run('dsdf_render_forward_grad', _ptr(tpad), tp, _ptr(out), _ptr(img), _ptr(ws), ws.numel())
    return (out, img) if return_image else out


# ---- multi-GPU pixel-tile split of a view (include/dsdf.h; driver: dsdf/parallel.py) ------------------------------------
def film_channels(integrator):
    return 4 if INTEGRATORS[integrator] == DSDF_DIRECT else 2


def new_film(n_views, W, H, integrator, device):
    """Zeroed film blocks (n_views, H+4, W+4, C)."""
    return torch.zeros(n_views, H + 4, W + 4, film_channels(integrator), dtype=torch.float32, device=device)


def render_film(grid, sensors, spp, film, rows, seeds=None, offsets=None, integrator=DSDF_SILHOUETTE, reparam=True,
                empty_space_skip=True, shading=None, emitter_samples=None, stats=None):
    """Primal samples of the film-block rows [rows[0], rows[1]) of every view, ACCUMULATED into `film`."""
    c = _Call(grid, sensors, spp, seeds, offsets, integrator, reparam, empty_space_skip, shading, emitter_samples)
    _require_dev(film, 'film')
    ws = c.workspace(False)
    c.run('dsdf_render_film', int(rows[0]), int(rows[1]), _ptr(film), _ptr(ws), ws.numel(), _ptr(stats))
    return film


def develop(film, W, H, integrator=DSDF_SILHOUETTE):
    """`HDRFilm.develop` of film blocks -> (n_views, H, W, 3)."""
    lib = _lib.load()
    _require_dev(film, 'film')
    nv = film.shape[0]
    img = torch.empty(nv, H, W, 3, dtype=torch.float32, device=film.device)
    with torch.cuda.device(film.device):
        _lib.check(lib.dsdf_develop(_ptr(film), nv, W, H, INTEGRATORS[integrator], _ptr(img), _stream()))
    return img


_sweep_workspaces = {}        # device -> {'ws': uint8 tensor, 'leased': bool}  (step_begin / step_finish)


class GradSweep:
    """The two halves of a gradient pass split at the film block: sweep() traces the window's samples (film accumulated,
    backward queue left in this object's workspace); after the films of all ranks were summed, backward() propagates the
    window's samples against the total film.  More than MAX_VIEWS_PER_LAUNCH sensors (the reference's default batch is all
    sensors of a config) are handled as consecutive parts of at most that many views, each with its own queue."""

    def __new__(cls, grid, sensors, *a, **kw):
        if len(_as_list(sensors)) > MAX_VIEWS_PER_LAUNCH and cls is GradSweep:
            return object.__new__(_GradSweepParts)
        return object.__new__(cls)

    def __init__(self, grid, sensors, spp, rows, seeds=None, offsets=None, integrator=DSDF_SILHOUETTE, reparam=True,
                 empty_space_skip=True, shading=None, emitter_samples=None, grad_albedo=None, workspace=None):
        c = self.call = _Call(grid, sensors, spp, seeds, offsets, integrator, reparam, empty_space_skip, shading, emitter_samples,
                              grad_albedo=grad_albedo)
        # the parameter block as it is NOW (sdf.p, warp settings): backward() may run after the caller touched grid.params
        c.params = type(grid.params).from_buffer_copy(grid.params)
        self.grid, self.nv = grid, c.nv
        self.rows = (int(rows[0]), int(rows[1]))
        wsb = self.ws_bytes = int(c.lib.dsdf_render_workspace_size(c.W, c.H, c.spp, c.nv, c.integrator))
        self.grid_version = None                              # set by sweep(): the grid the queue in `ws` belongs to
        # the backward queue lives in this buffer between the two halves: private to the sweep unless the caller lends one
        if workspace is not None and workspace.numel() >= wsb:
            self.ws = workspace
        else:
            self.ws = torch.empty(wsb, dtype=torch.uint8, device=grid.device)

    def _run(self, entry, *tail):
        c = self.call
        c.lib = self.grid.lib(c.extended)                     # (re-applies a general transform: state of the library instance)
        c.run(entry, *tail, _ptr(self.ws), self.ws.numel())

    def sweep(self, film):
        _require_dev(film, 'film')
        self.grid_version = self.grid.version
        self._run('dsdf_grad_sweep', self.rows[0], self.rows[1], _ptr(film))
        return film

    def make_private(self):
        """A workspace of its own for this sweep (a second backward of a step whose lent buffer went back to the pool)."""
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.grid.device)

    def backward(self, film_total, grad_image, grad_grid, grad_p=None):
        _require_dev(film_total, 'film_total'); grad_image = _require_dev(grad_image, 'grad_image'); _require_dev(grad_grid, 'grad_grid')
        c = self.call
        if grad_image.numel() != c.nv * c.H * c.W * 3:
            raise _lib.DsdfError(f"grad_image must be (n_views,H,W,3) = {(c.nv, c.H, c.W, 3)}, got {tuple(grad_image.shape)}")
        if self.grid_version != self.grid.version:
            # the padded buffer is rewritten in place by SdfGrid.update: the queued samples (warp points, records) belong to the
            # grid that was traced, the lookups of the backward would read the new one
            raise _lib.DsdfError("the grid was updated (SdfGrid.update / set_data) between the gradient sweep of this step and its "
                                 "backward: back-propagate before the optimiser step, or render again")
        self._run('dsdf_grad_backward', _ptr(film_total), _ptr(grad_image), _ptr(grad_grid), _ptr(grad_p))
        return grad_grid

    def record_stream(self, stream):
        self.ws.record_stream(stream)


class _GradSweepParts(GradSweep):
    """GradSweep over more sensors than one launch takes: consecutive parts with private workspaces."""

    def __init__(self, grid, sensors, spp, rows, seeds=None, offsets=None, emitter_samples=None, workspace=None, **kw):
        sensors = list(sensors)
        n, m = len(sensors), MAX_VIEWS_PER_LAUNCH
        W, H = sensors[0].film_size()
        n_lanes = (W + 4) * (H + 4) * int(spp)
        if seeds is not None and isinstance(seeds, int):
            seeds = [seeds] * n
        per_view = lambda t, a, b: None if t is None else t.reshape(n, n_lanes, 2)[a:b].contiguous()
        self.parts = [(a, min(a + m, n), GradSweep(grid, sensors[a:a + m], spp, rows, seeds=None if seeds is None else list(seeds)[a:a + m],
                                                   offsets=per_view(offsets, a, a + m), emitter_samples=per_view(emitter_samples, a, a + m), **kw))
                      for a in range(0, n, m)]
        self.nv, self.ws = n, None

    def sweep(self, film):
        for a, b, part in self.parts:
            part.sweep(film[a:b])
        return film

    def backward(self, film_total, grad_image, grad_grid, grad_p=None):
        for a, b, part in self.parts:
            part.backward(film_total[a:b], grad_image[a:b], grad_grid, grad_p)
        return grad_grid

    def record_stream(self, stream):
        for _, _, part in self.parts:
            part.ws.record_stream(stream)

    def make_private(self):
        for _, _, part in self.parts:
            part.make_private()


_side_streams = {}
_skip_buffers = {}


class StepHandle:
    """What step_begin leaves for step_finish: the gradient sweep (its workspace holds the backward queue and the adjoint
    coefficients), its film, and the streams to join."""

    def __init__(self, sweep, film_g, main, side, lease):
        self.sweep, self.film_g, self.main, self.side, self.lease = sweep, film_g, main, side, lease
        self.done = False


def share_proof_open(grid, shading, flags):
    """Opens the bracket in which the render calls of this thread that see the same grid, sensors and film size share ONE per-pixel
    proof (include/dsdf.h: dsdf_share_pixel_skip): the first computes the flags into `flags` (uint8, one per film-block pixel and
    view), the others wait for it and read them.  Returns the library the bracket is open on, for share_proof_close."""
    lib = grid.lib(_needs_extended(shading))
    with torch.cuda.device(grid.device):
        _lib.check(lib.dsdf_share_pixel_skip(_ptr(flags), flags.numel()))
    return lib


def share_proof_close(grid, lib):
    with torch.cuda.device(grid.device):
        lib.dsdf_share_pixel_skip(None, 0)


@contextlib.contextmanager
def shared_proof(grid, shading, flags):
    """The bracket of share_proof_open / share_proof_close around a block of render calls."""
    lib = share_proof_open(grid, shading, flags)
    try:
        yield
    finally:
        share_proof_close(grid, lib)


def _lease_sweep_workspace(dev):
    """The cached sweep workspace of `dev` unless a step that has begun and not yet finished still owns its queue."""
    ent = _sweep_workspaces.get(dev)
    if ent is None or ent['leased']:
        return None, None
    ent['leased'] = True
    return ent['ws'], ent


def step_begin(grid, sensors, spp, spp_grad, seeds, seeds_grad, integrator=DSDF_SILHOUETTE, reparam=True, shading=None,
               grad_albedo=None, empty_space_skip=True):
    """Forward half of one differentiable render step (python/shape_opt.py:77-80: `mi.render(..., seed, spp, seed_grad, spp_grad)`):
    returns (images, handle).  The forward sweep of the gradient pass (tracing, film, backward queue, the image-independent half
    of the adjoint: dsdf_grad_sweep) does not depend on the image gradient, so it is enqueued on a high-priority side stream
    beside the primal render; both passes share one empty-space / hit proof (dsdf_share_pixel_skip).  step_finish(handle,
    grad_image, ...) then runs what is left of the backward (dsdf_grad_backward).  This is the autograd boundary of the render
    op: torch's forward() calls step_begin, backward() calls step_finish."""
    sensors = _as_list(sensors)
    W, H = sensors[0].film_size()
    dev = grid.device
    main = torch.cuda.current_stream(dev)
    side = _side_streams.get(dev)
    if side is None:
        # high priority: the sweep's workers get the wave slots first, so it finishes early and its latency-bound tail kernel
        # (a handful of 1000-step rays) runs beside the bulk of the primal pass instead of after it
        side = _side_streams[dev] = torch.cuda.Stream(dev, priority=-1)
    side.wait_stream(main)                                    # the grid (and whatever produced it) is ready
    # one per-pixel proof for both passes (dsdf_share_pixel_skip): the sweep writes the flags, the primal render reads them
    # (two planes: the flags a caller may read, and behind them the library's effective plane of the third proof stage)
    nflag = 2 * len(sensors) * (W + 4) * (H + 4)
    flags = _skip_buffers.get(dev)
    if flags is None or flags.numel() < nflag:
        flags = _skip_buffers[dev] = torch.empty(nflag, dtype=torch.uint8, device=dev)
    # (DSDF_SHARE_SKIP=0, INTEGRATION.md: a proof per pass -- the tests compare the shared flags with that path)
    share = os.environ.get('DSDF_SHARE_SKIP', '1') != '0'
    with torch.cuda.device(dev), (shared_proof(grid, shading, flags) if share else contextlib.nullcontext()):
        ws, lease = _lease_sweep_workspace(dev)
        with torch.cuda.stream(side):
            sweep = GradSweep(grid, sensors, spp_grad, (0, H + 4), seeds=seeds_grad, integrator=integrator, reparam=reparam,
                              shading=shading, grad_albedo=grad_albedo, workspace=ws, empty_space_skip=empty_space_skip)
            if sweep.ws is not None and sweep.ws is not ws:
                if lease is not None:
                    lease['leased'] = False
                # (a larger / first buffer: it becomes the cached one, owned by this step until step_finish)
                lease = _sweep_workspaces[dev] = {'ws': sweep.ws, 'leased': True}
            film_g = sweep.sweep(new_film(len(sensors), W, H, integrator, dev))
        img = render_forward(grid, sensors, spp, seeds=seeds, integrator=integrator, reparam=reparam, shading=shading,
                             empty_space_skip=empty_space_skip)
    return img, StepHandle(sweep, film_g, main, side, lease)


def step_finish(handle, grad_image, grad_grid, grad_p=None):
    """Backward half of the step: waits for the side stream and back-propagates the queued samples of the sweep against
    `grad_image` (n,H,W,3) into grad_grid (and grad_p, and the albedo / roughness gradients the sweep was built with)."""
    if handle.done:
        # a second backward of the same step (retain_graph=True, torch.autograd.grad twice): the lent workspace went back to the
        # pool with the first one, so the sweep is traced again into a buffer of its own -- sequentially, on the caller's stream
        sw = handle.sweep
        sw.make_private()
        film = sw.sweep(torch.zeros_like(handle.film_g))
        sw.backward(film, grad_image.contiguous(), grad_grid, grad_p)
        return grad_grid
    cur = torch.cuda.current_stream(grad_grid.device)
    cur.wait_stream(handle.side)
    handle.film_g.record_stream(cur); handle.sweep.record_stream(cur)
    try:
        handle.sweep.backward(handle.film_g, grad_image.contiguous(), grad_grid, grad_p)
    finally:
        handle.done = True
        if handle.lease is not None:
            handle.lease['leased'] = False    # (the next sweep is stream-ordered after this backward; also when it was refused)
    return grad_grid


def render_step(grid, sensors, spp, spp_grad, loss_grad, grad_grid, seeds, seeds_grad, integrator=DSDF_SILHOUETTE, reparam=True,
                shading=None, grad_albedo=None, grad_p=None, overlap=True, empty_space_skip=True):
    """One differentiable render step (python/shape_opt.py:77-83 for a batch of views): primal render at `spp`, image
    gradient `loss_grad(images)`, gradient pass at `spp_grad` accumulating into `grad_grid` -- the same three library calls as
    render_forward + render_backward, scheduled on TWO HIP streams (step_begin / step_finish): only the backward proper
    (dsdf_grad_backward) waits for both the primal image and the sweep.  Returns the images."""
    sensors = _as_list(sensors)
    if not overlap:
        img = render_forward(grid, sensors, spp, seeds=seeds, integrator=integrator, reparam=reparam, shading=shading,
                             empty_space_skip=empty_space_skip)
        render_backward(grid, sensors, spp_grad, loss_grad(img), grad_grid=grad_grid, seeds=seeds_grad, integrator=integrator,
                        reparam=reparam, shading=shading, grad_albedo=grad_albedo, grad_p=grad_p, empty_space_skip=empty_space_skip)
        return img
    img, h = step_begin(grid, sensors, spp, spp_grad, seeds, seeds_grad, integrator, reparam, shading, grad_albedo, empty_space_skip)
    step_finish(h, loss_grad(img), grad_grid, grad_p)
    return img


def redistance(phi, return_status=False, return_counters=False):
    """`redistancing.redistance`: signed distance field with the zero level set of phi (Z,Y,X[,1]).  return_status: also a
    device int32 tensor, 0 = converged, 1 = the launch budget ran out first (read it when you synchronise anyway).
    return_counters: instead a device int32[4] = {rounds that did work, tile visits, Jacobi passes, status}."""
    lib = _lib.load()
    shape = phi.shape
    p3 = phi[..., 0] if phi.dim() == 4 else phi
    p3 = _require_dev(p3.detach(), 'phi')
    rz, ry, rx = (int(s) for s in p3.shape)
    out = torch.empty_like(p3)
    wsb = lib.dsdf_redistance_workspace_size(rx, ry, rz)
    ws = torch.empty(int(wsb), dtype=torch.uint8, device=p3.device)
    with torch.cuda.device(p3.device):
        _lib.check(lib.dsdf_redistance(_ptr(p3), rx, ry, rz, _ptr(out), _ptr(ws), wsb, _stream()))
        if return_counters:
            cnt = torch.zeros(4, dtype=torch.int32, device=p3.device)
            _lib.check(lib.dsdf_redistance_counters(_ptr(ws), rx, ry, rz, _ptr(cnt), _stream()))
            return out.reshape(shape), cnt
        if return_status:
            status = torch.zeros(1, dtype=torch.int32, device=p3.device)
            _lib.check(lib.dsdf_redistance_status(_ptr(ws), rx, ry, rz, _ptr(status), _stream()))
            return out.reshape(shape), status
    return out.reshape(shape)


def mesh_raycast(triangles, rays_o, rays_d, t_min=0.0):
    """Closest hit of rays against a triangle soup (T,3,3) -> (t (n,), backface (n,) int32): what `mesh_to_sdf.create_sdf`
    takes from `scene.ray_intersect` (python/mesh_to_sdf.py:24-26, 45)."""
    lib = _lib.load()
    tri = _require_dev(triangles.reshape(-1, 9), 'triangles')
    rays_o = _require_dev(rays_o, 'rays_o'); rays_d = _require_dev(rays_d, 'rays_d')
    n = rays_o.shape[0]
    t = torch.empty(n, dtype=torch.float32, device=rays_o.device)
    back = torch.empty(n, dtype=torch.int32, device=rays_o.device)
    with torch.cuda.device(rays_o.device):
        _lib.check(lib.dsdf_mesh_raycast(_ptr(tri), int(tri.shape[0]), _ptr(rays_o), _ptr(rays_d), n, C.c_float(t_min), _ptr(t), _ptr(back),
                                         _stream()))
    return t, back


class MeshBvh:
    """A bounding-volume hierarchy over a triangle soup in one device buffer (include/dsdf.h: the layout is ABI): Morton codes of
    the centroids (dsdf_mesh_morton), a stable torch sort -- plumbing -- and the build (dsdf_mesh_bvh_build).  `triangles`
    (T,3,3) and the optional per-corner `normals` (T,3,3) are device tensors; with normals the mesh renders smooth-shaded.
    `colors` (T,3,3): a linear reflectance (rgb) per triangle corner, kept beside the buffer as `.colors` in the caller's triangle order
    (the kernel looks them up by original index); dsdf.mesh_render shades sdf_direct_reparam with them instead of a reflectance volume."""

    def __init__(self, triangles, normals=None, colors=None):
        lib = _lib.load()
        tri = _require_dev(triangles.reshape(-1, 9), 'triangles')
        T = int(tri.shape[0])
        if T < 1:
            raise _lib.DsdfError("MeshBvh needs at least one triangle")
        nrm = None
        if normals is not None:
            nrm = _require_dev(normals.reshape(-1, 9), 'normals')
            if nrm.shape[0] != T:
                raise _lib.DsdfError(f"normals must be (T,3,3) like triangles, got {tuple(normals.shape)}")
        self.colors = None
        if colors is not None:
            if tuple(colors.shape) != (T, 3, 3):
                raise _lib.DsdfError(f"colors must be (T,3,3) like triangles, got {tuple(colors.shape)}")
            self.colors = _require_dev(colors, 'colors')
            if self.colors.device != tri.device:
                raise _lib.DsdfError("colors must live on the device of the triangles")
        self.device, self.n_triangles, self.has_normals = tri.device, T, nrm is not None
        self.triangles = tri.reshape(T, 3, 3)        # (the caller's order: what mesh_distance samples)
        self.moments = None                          # (the per-node moments of `winding`, built on first use)
        self.buffer = torch.empty(int(lib.dsdf_mesh_bvh_size(T, int(nrm is not None))), dtype=torch.float32, device=tri.device)
        codes = torch.empty(T, dtype=torch.int32, device=tri.device)
        with torch.cuda.device(tri.device):
            _lib.check(lib.dsdf_mesh_morton(_ptr(tri), T, _ptr(codes), _stream()))
            self.order = torch.sort(codes, stable=True).indices.to(torch.int32)
            _lib.check(lib.dsdf_mesh_bvh_build(_ptr(tri), _ptr(nrm), _ptr(self.order), T, _ptr(self.buffer), _stream()))

    def raycast(self, rays_o, rays_d, t_min=0.0, return_prim=False):
        """mesh_raycast through the hierarchy: (t, backface[, prim]) -- bit for bit the brute-force result; prim is the index of
        the hit triangle in `triangles`, -1 on a miss."""
        lib = _lib.load()
        rays_o = _require_dev(rays_o, 'rays_o'); rays_d = _require_dev(rays_d, 'rays_d')
        n = rays_o.shape[0]
        t = torch.empty(n, dtype=torch.float32, device=rays_o.device)
        back = torch.empty(n, dtype=torch.int32, device=rays_o.device)
        prim = torch.empty(n, dtype=torch.int32, device=rays_o.device) if return_prim else None
        with torch.cuda.device(rays_o.device):
            _lib.check(lib.dsdf_mesh_bvh_raycast(_ptr(self.buffer), _ptr(rays_o), _ptr(rays_d), n, C.c_float(t_min), _ptr(t), _ptr(back),
                                                 _ptr(prim), _stream()))
        return (t, back, prim) if return_prim else (t, back)

    def closest(self, points, max_dist=float('inf'), return_prim=False, return_point=False, return_bary=False):
        """mesh_closest through the hierarchy (dsdf_mesh_bvh_closest): the same arguments, bit for bit the brute-force result."""
        return _closest(lambda lib, *a: lib.dsdf_mesh_bvh_closest(_ptr(self.buffer), *a), self.device, points, max_dist, return_prim,
                        return_point, return_bary)

    def winding(self, points, beta=2.0):
        """The generalized winding number of the mesh at `points` (N,3) -> (N,) float32, through the hierarchy (dsdf_mesh_bvh_winding): a
        subtree farther than beta x its radius counts as one dipole.  beta >= 1; float('inf') is the exact sum (mesh_winding up to the order
        of the terms); the default 2 stays within 0.1 of it.  The moments buffer is built on first use and kept on the object."""
        lib = _lib.load()
        pts = _points(points, self.device)
        if not float(beta) >= 1.0:
            raise _lib.DsdfError(f"dsdf_mesh_bvh_winding: beta must be >= 1, got {beta}")
        with torch.cuda.device(self.device):
            if self.moments is None:
                mom = torch.empty(int(lib.dsdf_mesh_bvh_moments_size(self.n_triangles)), dtype=torch.float32, device=self.device)
                _lib.check(lib.dsdf_mesh_bvh_moments(_ptr(self.buffer), self.n_triangles, _ptr(mom), _stream()))
                self.moments = mom
            w = torch.empty(int(pts.shape[0]), dtype=torch.float32, device=self.device)
            _lib.check(lib.dsdf_mesh_bvh_winding(_ptr(self.buffer), _ptr(self.moments), _ptr(pts), int(pts.shape[0]), C.c_float(beta), _ptr(w),
                                                 _stream()))
        return w

    def signed_distance(self, points, beta=2.0):
        """The signed distance of `points` (N,3) to the mesh from two queries: `closest`, negated where `winding(points, beta)` > 0.5 (the
        renderer's convention: negative inside)."""
        d = self.closest(points)
        return torch.where(self.winding(points, beta) > 0.5, -d, d)


def _points(points, device):
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise _lib.DsdfError(f"points must be (N,3), got {tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__}")
    pts = _require_dev(points, 'points')
    if pts.device != device:
        raise _lib.DsdfError("points must live on the device of the mesh")
    return pts


def _closest(entry, device, points, max_dist, return_prim, return_point, return_bary):
    lib = _lib.load()
    pts = _points(points, device)
    n = int(pts.shape[0])
    dist = torch.empty(n, dtype=torch.float32, device=device)
    prim = torch.empty(n, dtype=torch.int32, device=device) if return_prim else None
    point = torch.empty(n, 3, dtype=torch.float32, device=device) if return_point else None
    bary = torch.empty(n, 2, dtype=torch.float32, device=device) if return_bary else None
    with torch.cuda.device(device):
        _lib.check(entry(lib, _ptr(pts), n, C.c_float(max_dist), _ptr(dist), _ptr(prim), _ptr(point), _ptr(bary), _stream()))
    out = (dist,) + tuple(t for t in (prim, point, bary) if t is not None)
    return out[0] if len(out) == 1 else out


def mesh_closest(triangles, points, max_dist=float('inf'), return_prim=False, return_point=False, return_bary=False):
    """Closest point of a triangle soup (T,3,3) to each of `points` (N,3), every point against every triangle (dsdf_mesh_closest; small
    meshes -- MeshBvh.closest serves large ones with the same bits) -> dist (N,), +inf where no triangle lies within max_dist (closed), or a
    tuple with, in this order, prim (N,) int32: the index of the closest triangle (-1: none; the lower one on equal distance), point (N,3):
    the closest point p0 + u e1 + v e2, bary (N,2): (u, v).  Exact for degenerate triangles too."""
    tri = _require_dev(triangles.reshape(-1, 9), 'triangles')
    if tri.shape[0] < 1:
        raise _lib.DsdfError("mesh_closest needs at least one triangle")
    return _closest(lambda lib, *a: lib.dsdf_mesh_closest(_ptr(tri), int(tri.shape[0]), *a), tri.device, points, max_dist, return_prim,
                    return_point, return_bary)


def mesh_winding(triangles, points):
    """The generalized winding number of a triangle soup (T,3,3) at `points` (N,3) -> (N,) float32: the exact sum of the signed solid angles
    over 4 pi, every point against every triangle (dsdf_mesh_winding; MeshBvh.winding serves large meshes).  1 inside an outward-oriented
    closed mesh, 0 outside; w > 0.5 is the inside test for an open or self-intersecting one."""
    lib = _lib.load()
    tri = _require_dev(triangles.reshape(-1, 9), 'triangles')
    if tri.shape[0] < 1:
        raise _lib.DsdfError("mesh_winding needs at least one triangle")
    pts = _points(points, tri.device)
    w = torch.empty(int(pts.shape[0]), dtype=torch.float32, device=tri.device)
    with torch.cuda.device(tri.device):
        _lib.check(lib.dsdf_mesh_winding(_ptr(tri), int(tri.shape[0]), _ptr(pts), int(pts.shape[0]), _ptr(w), _stream()))
    return w


BVH_MIN_TRIANGLES = 4096    # a mesh given as a tensor goes through a MeshBvh above this, through the brute-force kernels below (mesh_to_sdf shares it)


def mesh_signed_distance(mesh, points, beta=2.0):
    """The signed distance of `points` (N,3) to a mesh, negative inside: the `closest` distance, negated where the winding number exceeds
    0.5.  `mesh`: a MeshBvh, or (T,3,3) triangles -- above BVH_MIN_TRIANGLES (4096, the threshold of mesh_to_sdf) they go through a MeshBvh built
    for the call (`beta` as in MeshBvh.winding), below it through the two brute-force kernels (exact sum)."""
    if isinstance(mesh, MeshBvh):
        return mesh.signed_distance(points, beta)
    tri = _require_dev(mesh.reshape(-1, 9), 'mesh')
    if not float(beta) >= 1.0:
        raise _lib.DsdfError(f"mesh_signed_distance: beta must be >= 1, got {beta}")
    if tri.shape[0] > BVH_MIN_TRIANGLES:
        return MeshBvh(tri).signed_distance(points, beta)
    d = mesh_closest(tri, points)
    return torch.where(mesh_winding(tri, points) > 0.5, -d, d)


def sample_surface(triangles, n, seed=0):
    """`n` points uniform on the surface of a triangle soup (T,3,3) -> (points (n,3), prim (n,) int64, bary (n,2)): a triangle is drawn
    in proportion to its area (searchsorted on the cumulative areas, fp64), the point inside it by the square-root warp
    (u, v) = (sqrt(r1) (1 - r2), sqrt(r1) r2), point = p0 + u e1 + v e2.  Deterministic for a seed on a device.  Torch plumbing, no kernel.
    A triangle without area is never drawn; a mesh without area raises DsdfError."""
    tri = _require_dev(triangles.reshape(-1, 3, 3), 'triangles')
    dev = tri.device
    t64 = tri.double()
    e1, e2 = t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0]
    area = 0.5 * torch.linalg.norm(torch.linalg.cross(e1, e2), dim=1)
    cum = torch.cumsum(area, 0)
    total = float(cum[-1]) if cum.numel() else 0.0
    if not (total > 0.0 and total < float('inf')):
        raise _lib.DsdfError(f"sample_surface: the mesh has no surface to sample (total area {total})")
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    r = torch.rand(int(n), 3, dtype=torch.float64, device=dev, generator=gen)
    # right=True: the first triangle whose cumulative area EXCEEDS the draw, so one that adds nothing is never the answer
    prim = torch.searchsorted(cum, r[:, 0] * total, right=True).clamp_(max=int(torch.nonzero(area > 0)[-1]))
    s = torch.sqrt(r[:, 1])
    u, v = s * (1.0 - r[:, 2]), s * r[:, 2]
    pts = t64[prim, 0] + u[:, None] * e1[prim] + v[:, None] * e2[prim]
    return pts.float().contiguous(), prim, torch.stack([u, v], -1).float()


def mesh_distance(a, b, n=200_000, seed=0, threshold=None):
    """How far two surfaces are apart.  `a`, `b`: (T,3,3) triangles or MeshBvh objects (sampled from their `.triangles`).
    `n` points are sampled on each (sample_surface; seeds `seed` and `seed + 1`) and queried against the other mesh through its BVH ->
    a dict: a_to_b_mean / b_to_a_mean / a_to_b_max / b_to_a_max, chamfer_l1 = (a_to_b_mean + b_to_a_mean) / 2, chamfer_l2 = mean(d_ab^2) +
    mean(d_ba^2), hausdorff = the larger maximum (of the SAMPLED points: a lower bound of the true one); with `threshold`: precision and
    recall = the shares of d_ab and d_ba that are <= threshold, fscore = their harmonic mean (0 when both are 0); and the raw points_a,
    points_b, dist_a_to_b, dist_b_to_a (device tensors).  The statistics are accumulated in fp64."""
    def mesh(m, name):
        if isinstance(m, MeshBvh):
            return m.triangles, m
        tri = _require_dev(m.reshape(-1, 3, 3), name)
        return tri, MeshBvh(tri)
    (ta, ba), (tb, bb) = mesh(a, 'a'), mesh(b, 'b')
    pa, pb = sample_surface(ta, n, seed)[0], sample_surface(tb, n, int(seed) + 1)[0]
    dab, dba = bb.closest(pa), ba.closest(pb)
    d1, d2 = dab.double(), dba.double()
    out = {'a_to_b_mean': float(d1.mean()), 'b_to_a_mean': float(d2.mean()), 'a_to_b_max': float(d1.max()), 'b_to_a_max': float(d2.max())}
    out['chamfer_l1'] = (out['a_to_b_mean'] + out['b_to_a_mean']) / 2
    out['chamfer_l2'] = float((d1 * d1).mean()) + float((d2 * d2).mean())
    out['hausdorff'] = max(out['a_to_b_max'], out['b_to_a_max'])
    if threshold is not None:
        p, r = float((d1 <= float(threshold)).double().mean()), float((d2 <= float(threshold)).double().mean())
        out.update(precision=p, recall=r, fscore=2 * p * r / (p + r) if p + r > 0 else 0.0)
    out.update(points_a=pa, points_b=pb, dist_a_to_b=dab, dist_b_to_a=dba)
    return out


def mesh_render(bvh, sensors, spp, seeds=None, offsets=None, integrator=DSDF_SILHOUETTE, shading=None, emitter_samples=None,
                params=None):
    """Primal render of a triangle mesh (dsdf_mesh_render_forward): render_forward with the intersection routine swapped -- the
    reference images of a mesh scene (python/optimize.py:11-40) -> (n_views, H, W, 3).  `shading` (dsdf.Shading, diffuse, no
    use_mis) and `emitter_samples` belong to sdf_direct_reparam; `params` carries the clip planes and the light direction.
    A `bvh` with corner colours (MeshBvh(..., colors=)) takes the reflectance of sdf_direct_reparam from them
    (dsdf_mesh_render_forward_colors): shading.albedo is not read then and may be None."""
    lib = _lib.load()
    sensors, cams, W, H = _views(sensors)
    nv, spp = len(sensors), int(spp)
    n_lanes = (W + 4) * (H + 4) * spp
    offsets, cseeds = _sampler_args(nv, seeds, offsets, n_lanes)
    integ = INTEGRATORS[integrator]
    prm = params if params is not None else _lib.default_params()
    sh = keep = colors = None
    if integ == DSDF_DIRECT:
        if shading is None:
            raise _lib.DsdfError("sdf_direct_reparam needs shading=dsdf.Shading(albedo, ...)")
        colors = bvh.colors
        st, keep = shading.to_struct(nv, n_lanes, emitter_samples, need_albedo=colors is None)
        sh = C.byref(st)
    dev = bvh.device
    img = torch.empty(nv, H, W, 3, dtype=torch.float32, device=dev)
    ws = _workspace(dev, lib.dsdf_mesh_render_workspace_size(W, H, min(nv, MAX_VIEWS_PER_LAUNCH)), lib.dsdf_mesh_render_workspace_size(W, H, 1))
    with torch.cuda.device(dev):
        _lib.check(lib.dsdf_mesh_render_forward_colors(_ptr(bvh.buffer), _ptr(colors), C.byref(prm), cams, nv, W, H, spp, _ptr(offsets), cseeds,
                                                       integ, sh, _ptr(img), _ptr(ws), ws.numel(), _stream()))
    return img


def sample_volume(volume, points):
    """Trilinear lookup of a volume on the unit cube, (Z,Y,X,C) or (Z,Y,X) with C = 1 or 3, at `points` (N,3) in the volume's frame ->
    (N,C) (dsdf_volume_sample): the value the direct integrator reads there from a reflectance or roughness volume."""
    lib = _lib.load()
    vol = volume.detach()
    if vol.dim() == 3:
        vol = vol[..., None]
    if vol.dim() != 4 or vol.shape[3] not in (1, 3):
        raise _lib.DsdfError(f"volume must be (Z,Y,X) or (Z,Y,X,C) with C = 1 or 3, got {tuple(volume.shape)}")
    vol = _require_dev(vol, 'volume')
    if points.dim() != 2 or points.shape[1] != 3:
        raise _lib.DsdfError(f"points must be (N,3), got {tuple(points.shape)}")
    pts = _require_dev(points, 'points')
    vz, vy, vx, ch = (int(v) for v in vol.shape)
    n = int(pts.shape[0])
    out = torch.empty(n, ch, dtype=torch.float32, device=vol.device)
    with torch.cuda.device(vol.device):
        _lib.check(lib.dsdf_volume_sample(_ptr(vol), vx, vy, vz, ch, _ptr(pts), n, _ptr(out), _stream()))
    return out


def extract_mesh(grid, resolution=None, iso=0.0, steps=24, normals=True, colors=None):
    """Triangle mesh of the surface the renderer sees: the level set {f = iso} of the grid's tricubic lookup f, by marching tetrahedra
    on a lattice of `resolution` (an int or (nx, ny, nz); default: the grid's own) cells, every vertex moved onto the root of f on its
    lattice edge by `steps` bisection steps (include/dsdf.h: dsdf_iso_*, csrc/dsdf_iso.h) -> (vertices (V, 3) float32, faces (F, 3)
    int32[, normals (V, 3)]) on the grid's device, in WORLD space: the library works in the cube's own frame, `+ sdf.p` and a general
    to_world (normals through its inverse transpose) are applied here.  Faces wind so that their normal points towards larger f.
    `vertices[faces.long()]` with `normals[faces.long()]` is what dsdf.MeshBvh takes.  A surface that leaves the cube stays open there;
    no surface gives V = F = 0.  `colors`: a reflectance volume (Z,Y,X,3) on the device -- the tuple gains a last element (V, 3), its
    trilinear lookup (sample_volume) at the WORLD-space vertices returned (the volume lives in world space: what the direct integrator
    reads at that point of the surface).  The two exclusive scans between the launches are torch.cumsum (plumbing), and their totals are read
    back once to size the outputs -- the call synchronises there."""
    lib = _lib.load()                                      # (cube coordinates in either build: the default one serves every grid)
    if resolution is None:
        nx, ny, nz = grid.rx, grid.ry, grid.rz
    elif isinstance(resolution, (tuple, list)):
        nx, ny, nz = (int(v) for v in resolution)
    else:
        nx = ny = nz = int(resolution)
    dev = grid.device
    N = (nx + 1) * (ny + 1) * (nz + 1) if min(nx, ny, nz) >= 1 else 1
    iso_c = C.c_float(iso)
    with torch.cuda.device(dev):
        st = _stream()
        values = torch.empty(N, dtype=torch.float32, device=dev)
        _lib.check(lib.dsdf_iso_sample(_ptr(grid.padded), grid.rx, grid.ry, grid.rz, nx, ny, nz, _ptr(values), st))
        cross = torch.empty(N, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, N, dtype=torch.int32, device=dev)
        _lib.check(lib.dsdf_iso_mark(_ptr(values), nx, ny, nz, iso_c, _ptr(cross), _ptr(counts[0]), _ptr(counts[1]), st))
        # (one 1-D scan per count: a scan along the rows of a (2, N) tensor runs one block per row, 350 x slower at 256^3)
        ends = torch.stack([torch.cumsum(counts[0], 0, dtype=torch.int32), torch.cumsum(counts[1], 0, dtype=torch.int32)])
        V, F = (int(v) for v in ends[:, -1].tolist())
        offsets = ends - counts
        vert_edge = torch.empty(V, dtype=torch.int32, device=dev)
        faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
        pos = torch.empty(V, 3, dtype=torch.float32, device=dev)
        nrm = torch.empty(V, 3, dtype=torch.float32, device=dev) if normals else None
        if V > 0:
            _lib.check(lib.dsdf_iso_emit(_ptr(values), nx, ny, nz, iso_c, _ptr(cross), _ptr(offsets[0]), _ptr(offsets[1]), _ptr(vert_edge),
                                         _ptr(faces), st))
            _lib.check(lib.dsdf_iso_refine(_ptr(grid.padded), grid.rx, grid.ry, grid.rz, _ptr(values), nx, ny, nz, iso_c, _ptr(vert_edge), V,
                                           int(steps), _ptr(pos), _ptr(nrm), st))
    if grid.transform is not None:
        tw = torch.as_tensor(grid.to_world, dtype=torch.float64, device=dev)
        pos = (pos.double() @ tw[:3, :3].T + tw[:3, 3]).float()
        if nrm is not None:
            nrm = torch.nn.functional.normalize(nrm.double() @ torch.linalg.inv(tw[:3, :3]), dim=1).float()
    pos = pos + torch.tensor([float(v) for v in grid.params.sdf_p], dtype=torch.float32, device=dev)
    out = (pos, faces, nrm) if normals else (pos, faces)
    if colors is not None:
        if colors.dim() != 4 or colors.shape[3] != 3:
            raise _lib.DsdfError(f"colors must be a reflectance volume (Z,Y,X,3), got {tuple(colors.shape)}")
        out += (sample_volume(colors, pos),)
    return out


SIMPLIFY_REG = 1e-3         # DSDF_SIMPLIFY_REG of csrc/dsdf_simplify.h
SIMPLIFY_GROW = 2.0 ** -13  # the default box of simplify_mesh: the mesh AABB grown by this share of its largest extent on every side


def resolve_cells(cells, lo, hi):
    """(cx, cy, cz) of simplify_mesh's `cells`: a triple as it is; an int = that many cells along the longest extent of the box lo / hi and
    cubic cells of that size on the other axes, ceil(extent / size), at least 1."""
    if isinstance(cells, (tuple, list)):
        c = tuple(int(v) for v in cells)
        if len(c) != 3 or min(c) < 1:
            raise _lib.DsdfError(f"cells must be an int >= 1 or three of them, got {cells!r}")
        return c
    n = int(cells)
    if n < 1:
        raise _lib.DsdfError(f"cells must be an int >= 1 or three of them, got {cells!r}")
    ext = [float(h) - float(l) for l, h in zip(lo, hi)]
    size = max(ext) / n
    return tuple(n if e == max(ext) else min(n, max(1, math.ceil(e / size))) for e in ext)


def simplify_mesh(vertices, faces, cells, bounds=None, normals=False, colors=None, reg=SIMPLIFY_REG):
    """Simplifies an indexed triangle mesh by vertex clustering with quadric error metrics (Lindstrom 2000; include/dsdf.h: dsdf_simplify_*,
    csrc/dsdf_simplify.h) -> (vertices' (V', 3) float32, faces' (F', 3) int32[, normals' (V', 3)][, colors' (V', 3)]) on the input's device.
    All vertices in one cell of a regular grid become one vertex, placed where the summed squared distance to the planes of the cell's
    triangles is smallest (regularised towards the mean of the cell's corners by `reg`) and clamped into the cell; a face whose corners do
    not end up in three different cells disappears.  vertices (V, 3) float32, faces (F, 3) int32 (int64 is converted).
    `cells`: (cx, cy, cz), or an int: that many along the longest extent of the box, cubic cells on the other axes.  `bounds` = (lo, hi): the
    box of the grid -- pass the same one for two meshes to put them on one grid; default: the AABB of `vertices` grown by 2^-13 of its
    largest extent (an axis without extent still has a box).  A vertex outside the box counts to the border cell.
    `normals=True`: the normalised area-weighted normal sum of each cell's triangles (zero where it vanishes); `colors` (V, 3): their mean
    over the cell's face corners.  Output vertices come in ascending cell order, output faces are the survivors in input order with their
    winding kept.  Every output face is an input face with its corners moved inside their cells, so the result lies within one cell
    diagonal of the input, and a closed input keeps its winding number at every point farther away than that.  Duplicate faces, and the
    opposite pairs a collapsing thin sheet leaves, are KEPT as they are, and non-manifold edges can appear.  No faces, or all of them
    collapsed: empty tensors of the right shapes.  The sort of the corner keys and the scans between the launches are torch (plumbing); the
    counts are read back to size the outputs -- the call synchronises there."""
    lib = _lib.load()
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise _lib.DsdfError(f"vertices must be (V,3), got {tuple(vertices.shape) if isinstance(vertices, torch.Tensor) else type(vertices).__name__}")
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.DsdfError(f"faces must be (F,3), got {tuple(faces.shape) if isinstance(faces, torch.Tensor) else type(faces).__name__}")
    vert = _require_dev(vertices, 'vertices')
    dev = vert.device
    if faces.dtype not in (torch.int32, torch.int64):
        raise _lib.DsdfError(f"faces must be int32 (or int64), got {faces.dtype}")
    fac = _require_dev(faces.to(torch.int32), 'faces', torch.int32)
    if fac.device != dev:
        raise _lib.DsdfError("faces must live on the device of the vertices")
    col = None
    if colors is not None:
        if not isinstance(colors, torch.Tensor) or tuple(colors.shape) != tuple(vert.shape):
            raise _lib.DsdfError(f"colors must be (V,3) like vertices, got {tuple(colors.shape) if isinstance(colors, torch.Tensor) else type(colors).__name__}")
        col = _require_dev(colors, 'colors')
        if col.device != dev:
            raise _lib.DsdfError("colors must live on the device of the vertices")
    if not (float(reg) > 0.0 and float(reg) < float('inf')):
        raise _lib.DsdfError(f"simplify_mesh: reg must be > 0, got {reg}")
    V, F = int(vert.shape[0]), int(fac.shape[0])
    if 3 * F >= 2 ** 31:
        raise _lib.DsdfError(f"simplify_mesh: {F} faces: 3 F must stay below 2^31")
    if F > 0 and (V == 0 or int(faces.min()) < 0 or int(faces.max()) >= V):
        raise _lib.DsdfError("simplify_mesh: face index out of range")
    if bounds is not None:
        lo, hi = ([float(v) for v in b] for b in bounds)
    elif V > 0:
        lo_t, hi_t = vert.amin(0).double(), vert.amax(0).double()
        grow = SIMPLIFY_GROW * float((hi_t - lo_t).max())
        lo, hi = (lo_t - grow).float().tolist(), (hi_t + grow).float().tolist()
        if not all(h > l for l, h in zip(lo, hi)):                 # a single point (or non-finite vertices): any box around it
            lo, hi = [l - 1.0 for l in lo], [h + 1.0 for h in hi]
    else:
        lo, hi = [0.0] * 3, [1.0] * 3
    if len(lo) != 3 or len(hi) != 3:
        raise _lib.DsdfError("bounds must be (lo, hi) with three numbers each")
    cx, cy, cz = resolve_cells(cells, lo, hi)
    lo_c, hi_c = (C.c_float * 3)(*lo), (C.c_float * 3)(*hi)
    empty = lambda dt=torch.float32: torch.empty(0, 3, dtype=dt, device=dev)
    result = lambda v, f, n, c: (v, f) + ((n,) if normals else ()) + ((c,) if colors is not None else ())
    with torch.cuda.device(dev):
        st = _stream()
        keys = torch.empty(3 * F, dtype=torch.int32, device=dev)
        _lib.check(lib.dsdf_simplify_keys(_ptr(vert), _ptr(fac), F, lo_c, hi_c, cx, cy, cz, _ptr(keys), st))       # (refuses a bad grid for F = 0 too)
        if F == 0:
            return result(empty(), empty(torch.int32), empty(), empty())
        sorted_keys, order = torch.sort(keys, stable=True)
        corner = order.to(torch.int32)
        cell_keys, counts = torch.unique_consecutive(sorted_keys, return_counts=True)
        U = int(cell_keys.shape[0])
        cell_start = torch.zeros(U + 1, dtype=torch.int32, device=dev)
        cell_start[1:] = torch.cumsum(counts, 0)
        rank = torch.empty(3 * F, dtype=torch.int32, device=dev)
        keep = torch.empty(F, dtype=torch.int32, device=dev)
        used = torch.zeros(U, dtype=torch.int32, device=dev)
        _lib.check(lib.dsdf_simplify_mark(_ptr(keys), F, _ptr(cell_keys), U, _ptr(rank), _ptr(keep), _ptr(used), st))
        v_end, f_end = torch.cumsum(used, 0, dtype=torch.int32), torch.cumsum(keep, 0, dtype=torch.int32)
        Vn, Fn = (int(v) for v in torch.stack([v_end[-1], f_end[-1]]).tolist())
        faces_out = torch.empty(Fn, 3, dtype=torch.int32, device=dev)
        pos = torch.empty(Vn, 3, dtype=torch.float32, device=dev)
        nrm = torch.empty(Vn, 3, dtype=torch.float32, device=dev) if normals else None
        col_out = torch.empty(Vn, 3, dtype=torch.float32, device=dev) if col is not None else None
        if Fn > 0:
            vertex_id, face_offset = v_end - used, f_end - keep
            _lib.check(lib.dsdf_simplify_emit(_ptr(vert), _ptr(fac), F, _ptr(col), lo_c, hi_c, cx, cy, cz, C.c_float(float(reg)), _ptr(corner),
                                              _ptr(cell_keys), _ptr(cell_start), U, _ptr(rank), _ptr(keep), _ptr(face_offset), _ptr(used),
                                              _ptr(vertex_id), _ptr(faces_out), _ptr(pos), _ptr(nrm), _ptr(col_out), st))
    return result(pos, faces_out, nrm, col_out)


class MeshComponents:
    """What mesh_components returns: n (C), label (V int32), face_component (F int32), vertex_component (V int32), faces_per_component
    (C int64) and, when vertices were given, area / volume (C float64), bbox (C, 2, 3 float32: lower and upper corner) and boundary_edges
    (C int64); the attributes that were not computed are None."""
    __slots__ = ('n', 'label', 'face_component', 'vertex_component', 'faces_per_component', 'area', 'volume', 'bbox', 'boundary_edges')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    def __repr__(self):
        return f"MeshComponents(n={self.n}, faces={0 if self.face_component is None else self.face_component.shape[0]})"


def _mesh_args(who, vertices, faces, n_vertices=None):
    """The checks simplify_mesh makes of an indexed mesh -> (vertices or None, int32 faces, V, F); `vertices` may be None here."""
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.DsdfError(f"faces must be (F,3), got {tuple(faces.shape) if isinstance(faces, torch.Tensor) else type(faces).__name__}")
    if faces.dtype not in (torch.int32, torch.int64):
        raise _lib.DsdfError(f"faces must be int32 (or int64), got {faces.dtype}")
    fac = _require_dev(faces.to(torch.int32), 'faces', torch.int32)
    vert = None
    if vertices is not None:
        if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
            raise _lib.DsdfError(f"vertices must be (V,3), got {tuple(vertices.shape) if isinstance(vertices, torch.Tensor) else type(vertices).__name__}")
        vert = _require_dev(vertices, 'vertices')
        if vert.device != fac.device:
            raise _lib.DsdfError("faces must live on the device of the vertices")
        if n_vertices is not None and int(n_vertices) != vert.shape[0]:
            raise _lib.DsdfError(f"{who}: n_vertices = {n_vertices}, but vertices has {vert.shape[0]} rows")
    F = int(fac.shape[0])
    if 3 * F >= 2 ** 31:
        raise _lib.DsdfError(f"{who}: {F} faces: 3 F must stay below 2^31")
    lo, hi = (int(faces.min()), int(faces.max())) if F > 0 else (0, -1)
    V = int(vert.shape[0]) if vert is not None else (int(n_vertices) if n_vertices is not None else hi + 1)
    if V < 0 or V >= 2 ** 31:
        raise _lib.DsdfError(f"{who}: n_vertices must be in [0, 2^31), got {V}")
    if F > 0 and (lo < 0 or hi >= V):
        raise _lib.DsdfError(f"{who}: face index out of range")
    return vert, fac, V, F


def mesh_components(faces, n_vertices=None, vertices=None, connect='index'):
    """Connected components of an indexed triangle mesh (include/dsdf.h: dsdf_mesh_components, a lock-free union-find over the index
    buffer; csrc/dsdf_components.h) -> MeshComponents on the input's device.  faces (F, 3) int32 (int64 is converted) with every index in
    [0, V); V = `n_vertices`, or the rows of `vertices`, or the largest index + 1.  Two vertices are connected when a face names both:
    by shared vertex INDEX, not by shared edge -- two triangles that touch in one vertex are one component.  `label[v]` is the smallest
    vertex index of v's component (a vertex that no face names is its own label); components are numbered 0 ... n - 1 in ascending order
    of their label, counting only components with a face: `face_component` in [0, n), `vertex_component` in [0, n) or -1 for a vertex that
    no face names; `faces_per_component`.
    With `vertices` (V, 3) float32 also per component: `area` and `volume` (float64 sums of the float32 terms of dsdf_mesh_face_measures:
    0.5 |(p1 - p0) x (p2 - p0)| and p0 . (p1 x p2) / 6), `bbox` over the corners of its faces, and `boundary_edges`: the number of
    undirected edges that exactly one face uses (that occur once among the sides of the faces; a side between equal indices is none).  A component with boundary_edges == 0 is CLOSED, and only then does `volume` mean a
    volume (signed: positive for outward faces); for an open component it depends on where the origin is.
    connect='position' (needs `vertices`) first merges vertices with equal coordinates (torch.unique over the rows), which covers a soup
    read from a file that repeats its vertices; labels, components and boundary edges are then those of the merged mesh, but every result
    is still indexed by -- and `label` still names -- the caller's own vertices and faces.
    The numbering is torch scans and the sums are torch index_add_ / scatter_reduce (plumbing); the number of components is read back to
    size the outputs -- the call synchronises there.  A status word the kernels set if a walk exceeds V + 1 steps (impossible on a valid
    index buffer) raises DsdfError."""
    lib = _lib.load()
    if connect not in ('index', 'position'):
        raise _lib.DsdfError(f"connect must be 'index' or 'position', got {connect!r}")
    vert, fac, V, F = _mesh_args('mesh_components', vertices, faces, n_vertices)
    if connect == 'position' and vert is None:
        raise _lib.DsdfError("mesh_components: connect='position' needs the vertices")
    dev = fac.device
    with torch.cuda.device(dev):
        st = _stream()
        own = torch.arange(V, dtype=torch.int64, device=dev)
        if connect == 'position':
            merged, inv = torch.unique(vert, dim=0, return_inverse=True)                  # inv (V,): the merged vertex of every vertex
            inv, Vw = inv.reshape(-1), int(merged.shape[0])
            work = inv[fac.long()].to(torch.int32).contiguous()
        else:
            inv, Vw, work = None, V, fac
        label = torch.empty(Vw, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.dsdf_mesh_components(_ptr(work), F, Vw, _ptr(label), _ptr(status), st))
        if inv is not None:                                       # back to the caller's numbering: the smallest of HIS indices in the component
            root = label.long()[inv]
            first = torch.full((Vw,), V, dtype=torch.int64, device=dev).scatter_reduce_(0, root, own, 'amin')
            label = first[root].to(torch.int32)
        lab = label.long()
        face_label = lab[fac[:, 0].long()]
        with_face = torch.zeros(V, dtype=torch.bool, device=dev)
        with_face[face_label] = True
        number = torch.cumsum(with_face, 0) - 1                   # (V,) int64: the component number at every label that has a face
        n_t = number[-1:] + 1 if V > 0 else torch.zeros(1, dtype=torch.int64, device=dev)
        n, bad = (int(v) for v in torch.cat([n_t, status.long()]).tolist())
        if bad:
            raise _lib.DsdfError("mesh_components: a walk through the labels did not end within V + 1 steps (dsdf_mesh_components gave up)")
        fc = number[face_label]
        out = MeshComponents(n=n, label=label, face_component=fc.to(torch.int32),
                             vertex_component=torch.where(with_face[lab], number[lab], -1).to(torch.int32) if V > 0 else label.clone(),
                             faces_per_component=torch.bincount(fc, minlength=n))
        if vert is None:
            return out
        area = torch.empty(F, dtype=torch.float32, device=dev)
        vol = torch.empty(F, dtype=torch.float32, device=dev)
        _lib.check(lib.dsdf_mesh_face_measures(_ptr(vert), _ptr(fac), F, _ptr(area), _ptr(vol), st))
        # The atomics of index_add_ / scatter_reduce_ serialise per address, and a mesh of one or two components sends every face to the
        # same one (measured: 173 ms for 279 148 faces in 2 components): face f of component c goes to slot c K + f % K, and a plain
        # reduction over the K slots of each component follows.
        K = max(1, min(1024, 8192 // max(n, 1)))
        slot = fc * K + torch.arange(F, dtype=torch.int64, device=dev) % K
        total = lambda t: torch.zeros(n * K, dtype=torch.float64, device=dev).index_add_(0, slot, t.double()).view(n, K).sum(1)
        out.area, out.volume = total(area), total(vol)
        corners = vert[fac.long().reshape(-1)]                    # (3 F, 3)
        idx = slot.repeat_interleave(3)[:, None].expand(-1, 3)
        lo = torch.full((n * K, 3), float('inf'), dtype=torch.float32, device=dev).scatter_reduce_(0, idx, corners, 'amin')
        hi = torch.full((n * K, 3), float('-inf'), dtype=torch.float32, device=dev).scatter_reduce_(0, idx, corners, 'amax')
        out.bbox = torch.stack([lo.view(n, K, 3).amin(1), hi.view(n, K, 3).amax(1)], 1)
        w = work.long()
        a, b = w.reshape(-1), w[:, [1, 2, 0]].reshape(-1)         # the edges (i0, i1), (i1, i2), (i2, i0) of every face
        key = torch.minimum(a, b) * max(Vw, 1) + torch.maximum(a, b)
        _, back, uses = torch.unique(key, return_inverse=True, return_counts=True)
        once = (uses[back] == 1) & (a != b) if F > 0 else torch.zeros(0, dtype=torch.bool, device=dev)
        out.boundary_edges = torch.bincount(fc.repeat_interleave(3)[once], minlength=n)
    return out


def filter_components(vertices, faces, keep=None, min_area=None, min_faces=None, normals=None, colors=None, connect='index', return_counts=False):
    """Drops whole connected components of an indexed mesh (mesh_components) -> (vertices', faces'[, normals'][, colors']) on the input's
    device.  `keep=k`: only the k components of largest area stay (equal areas: the smaller component number first); `min_area`,
    `min_faces`: only components with at least that area / that many faces stay; what is given combines by AND.  Faces stay in input
    order with their winding; vertices that no kept face names are dropped and the rest stay in input order, `normals` / `colors` (V, 3)
    with them.  Everything filtered away: empty tensors of the right shapes.  `connect` as in mesh_components; `return_counts=True` appends the pair (components found, components kept).  The areas are float64
    sums by atomic adds, whose last bit can depend on the order: two components whose areas agree to that bit may swap places."""
    if keep is not None and (isinstance(keep, bool) or not isinstance(keep, int) or keep < 1):
        raise _lib.DsdfError(f"filter_components: keep must be an int >= 1, got {keep!r}")
    if min_area is not None and not float(min_area) >= 0.0:
        raise _lib.DsdfError(f"filter_components: min_area must be >= 0, got {min_area!r}")
    if min_faces is not None and (isinstance(min_faces, bool) or not isinstance(min_faces, int) or min_faces < 0):
        raise _lib.DsdfError(f"filter_components: min_faces must be an int >= 0, got {min_faces!r}")
    if vertices is None:
        raise _lib.DsdfError("vertices must be (V,3), got NoneType")
    vert, fac, V, F = _mesh_args('filter_components', vertices, faces)
    extras = []
    for name, t in (('normals', normals), ('colors', colors)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(vert.shape):
            raise _lib.DsdfError(f"{name} must be (V,3) like vertices, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
        t = _require_dev(t, name)
        if t.device != vert.device:
            raise _lib.DsdfError(f"{name} must live on the device of the vertices")
        extras.append(t)
    comp = mesh_components(fac, vertices=vert, connect=connect)
    dev = vert.device
    ok = torch.ones(comp.n, dtype=torch.bool, device=dev)
    if min_area is not None:
        ok &= comp.area >= float(min_area)
    if min_faces is not None:
        ok &= comp.faces_per_component >= int(min_faces)
    if keep is not None:
        largest = torch.sort(comp.area, descending=True, stable=True)[1][:keep]
        top = torch.zeros(comp.n, dtype=torch.bool, device=dev)
        top[largest] = True
        ok &= top
    face_stays = ok[comp.face_component.long()]
    kept = fac[face_stays]
    vertex_stays = torch.zeros(V, dtype=torch.bool, device=dev)
    vertex_stays[kept.long().reshape(-1)] = True
    new_id = (torch.cumsum(vertex_stays, 0) - 1).to(torch.int32)
    out = (vert[vertex_stays], new_id[kept.long()].reshape(-1, 3)) + tuple(t[vertex_stays] for t in extras)
    return out + ((comp.n, int(ok.sum())),) if return_counts else out


def kernel_timing_arm():
    """Measurement hook (include/dsdf.h): the next render call brackets its render kernel with HIP events."""
    _lib.check(_lib.load().dsdf_kernel_timing_arm())


def kernel_timing_read():
    """Milliseconds the render kernel of the call after kernel_timing_arm() took (waits for it)."""
    ms = C.c_float(0.0)
    _lib.check(_lib.load().dsdf_kernel_timing_read(C.byref(ms)))
    return float(ms.value)


def tail_stats_arm(stats):
    """Measurement hook (include/dsdf.h: dsdf_tail_stats_arm): the tail kernels of this thread's later calls that pass no `stats`
    of their own write their wave diagnostics into `stats` (new_stats(); None disarms).  Read them with stats_dict().
    The library keeps the raw pointer until it is disarmed: the tensor is held here so that it cannot be freed under an armed hook.
    (Variant libraries loaded AFTER this call are not armed.)"""
    global _tail_stats_held
    if stats is not None and (stats.dtype != torch.int64 or stats.numel() < 64 * STAT_SLOTS or not stats.is_contiguous()):
        raise ValueError("tail_stats_arm: a contiguous int64 tensor of 64 x STAT_SLOTS counters (new_stats()) is expected")
    for lib in {id(l): l for l in (_lib.load(), *_lib._variants.values())}.values():
        _lib.check(lib.dsdf_tail_stats_arm(_ptr(stats) if stats is not None else None))
    _tail_stats_held = stats


_tail_stats_held = None


def new_stats(device):
    return torch.zeros(64, STAT_SLOTS, dtype=torch.int64, device=device)


def stats_dict(stats):
    """Sums the 64 interleaved copies.  `steps` / `wave_steps` count the render kernel only; `all_steps` adds what the tail
    kernels marched for the rays handed over to them."""
    tot = [int(x) for x in stats.sum(0).cpu()]
    d = dict(zip(STAT_NAMES, tot))
    d['all_steps'] = d['steps'] + d['tail_steps']
    # the tail waves of the call (csrc/dsdf_tail.h: tail_stats; meaningful for ONE tail launch per buffer)
    rows = [[int(x) for x in stats[r].cpu()] for r in range(4)]
    r0, r1 = rows[0], rows[1]
    d['tail_waves'] = {'max_wave_steps': r0[11], 'max_us': r0[12] / 100.0, 'sum_us': r0[13] / 100.0, 'sum_clocks': r0[14],
                       'sum_refill_clocks': r0[15], 'refills': r1[11], 'clocks_completing': r1[12], 'clocks_claiming': r1[13],
                       'clocks_setting_up': r1[14], 'idle_lanes_at_refill': r1[15]}
    M = (1 << 64) - 1
    for name, r in (('primal_tail', rows[2]), ('sweep_tail', rows[3])):
        if r[12]:                           # wall-clock ticks (10 ns), relative to the earliest wave start of the kernel
            t0 = M - (r[11] & M)             # (the tensor is int64: the complemented minima read back negative)
            d['tail_waves'][name] = {'latest_start_us': (r[12] - t0) / 100.0, 'earliest_end_us': ((M - (r[13] & M)) - t0) / 100.0,
                                     'latest_end_us': (r[14] - t0) / 100.0, 'first_start_tick': t0}
    return d


def eager_sweep_enabled():
    """DSDF_EAGER_SWEEP=0: the autograd render ops do NOT enqueue the gradient sweep in forward() -- backward() then runs a plain
    sequential gradient pass.  Default 1 (the optimiser loop's fast path).  What the eager schedule costs, so that a caller can
    decide: a grad-enabled render that is never back-propagated (a validation image rendered without torch.no_grad()) pays a
    gradient sweep it does not need, and every render whose backward is still outstanding keeps its backward queue (40 B per
    gradient-pass sample and view: 8.2 GB + 8.2 GB of coefficients for 12 views x 512^2 x 64 spp) until its backward ran or
    its graph is freed; several such renders hold a queue each (the first leases the cached buffer, the others allocate)."""
    return os.environ.get('DSDF_EAGER_SWEEP', '1') != '0'


class _RenderOp(torch.autograd.Function):
    """`mi.render`'s custom op: primal (seed, spp) without AD, backward via an independent (seed_grad, spp_grad) gradient
    pass -- split at the autograd boundary like dsdf.render_step: forward() enqueues the primal render AND the image-independent
    sweep of the gradient pass (two streams, step_begin), backward() only what needs the image gradient (step_finish)."""

    @staticmethod
    def forward(ctx, data, grid, sensors, spp, seed, spp_grad, seed_grad, integrator, reparam, p=None, albedo=None,
                shading=None, roughness=None):
        if albedo is not None:
            shading = shading.with_albedo(albedo)
        ctx.data_shape = data.shape
        ctx.p_meta = None if p is None else (p.shape, p.dtype, p.device)
        if not grid.in_sync_with(data):                      # the caller stepped `data` without grid.update(): rebuild the padded copy
            grid.update(data)
        if p is not None:
            grid.set_translation(p)
        n = len(sensors)
        sh = shading
        want_r = sh is not None and sh.roughness is not None and roughness is not None and ctx.needs_input_grad[12]
        want_a = sh is not None and (ctx.needs_input_grad[10] or want_r)         # (the library scatters both volumes in one call)
        ctx.ga = torch.zeros_like(sh.albedo.detach(), dtype=torch.float32).contiguous() if want_a else None
        ctx.gr = None
        if want_r:
            ctx.gr = sh.grad_roughness = torch.zeros_like(sh.roughness.detach(), dtype=torch.float32).contiguous()
        ctx.gp = torch.zeros(3, dtype=torch.float32, device=grid.device) if (p is not None and ctx.needs_input_grad[9]) else None
        ctx.grid = grid
        ctx.version = grid.version                           # the grid state this render saw: backward() refuses any other
        ctx.n_backward = 0
        if not eager_sweep_enabled():
            ctx.step = None
            ctx.lazy = (list(sensors), int(spp_grad), [seed_grad + i for i in range(n)], integrator, reparam, sh, grid.version)
            return render_forward(grid, sensors, spp, seeds=[seed + i for i in range(n)], integrator=integrator, reparam=reparam, shading=sh)
        img, ctx.step = step_begin(grid, sensors, spp, spp_grad, [seed + i for i in range(n)], [seed_grad + i for i in range(n)],
                                   integrator, reparam, sh, ctx.ga)
        return img

    @staticmethod
    def backward(ctx, grad_out):
        #  every path -- the lazy one, the eager step_finish and its re-trace for a second backward, which would
        # otherwise stamp the sweep with the CURRENT grid version -- differentiates the grid state the forward pass rendered
        if ctx.version != ctx.grid.version:
            raise _lib.DsdfError("the grid was updated between this render and its backward: back-propagate before the optimiser step")
        # the kernels ACCUMULATE into gp / ga / gr (atomics): a second backward (retain_graph=True) starts from zero again, and what
        # a backward returns are copies -- the accumulators of this op are never handed out
        if ctx.n_backward > 0:
            for t in (ctx.gp, ctx.ga, ctx.gr):
                if t is not None:
                    t.zero_()
        ctx.n_backward += 1
        g = torch.zeros(ctx.grid.shape, dtype=torch.float32, device=ctx.grid.device)
        if ctx.step is None:
            sensors, spp_grad, seeds_grad, integrator, reparam, sh, ver = ctx.lazy
            render_backward(ctx.grid, sensors, spp_grad, grad_out.contiguous(), grad_grid=g, seeds=seeds_grad, integrator=integrator,
                            reparam=reparam, grad_p=ctx.gp, shading=sh, grad_albedo=ctx.ga)
        else:
            step_finish(ctx.step, grad_out, g, ctx.gp)
        gp = ctx.gp
        if gp is not None:
            shape, dtype, dev = ctx.p_meta
            gp = gp.to(device=dev, dtype=dtype).reshape(shape).clone()
        return (g.reshape(ctx.data_shape) if ctx.needs_input_grad[0] else None, None, None, None, None, None, None,
                None, None, gp, ctx.ga.clone() if (ctx.ga is not None and ctx.needs_input_grad[10]) else None, None,
                None if ctx.gr is None else ctx.gr.clone())


def render(data, grid, sensors, spp, seed=0, spp_grad=None, seed_grad=0, integrator=DSDF_SILHOUETTE, reparam=True,
           p=None, shading=None):
    """Differentiable render of `data` (the tensor behind `grid`) for one or more
    sensors: returns (n_views,H,W,3) attached to `data` and, if given, to the
    translation `p` (3,) (`SamplingIntegrator.sdf.p`)."""
    sensors = _as_list(sensors)
    albedo = shading.albedo if shading is not None else None      # attached when it requires grad (sdf_direct_reparam)
    rough = shading.roughness if shading is not None else None    # ... and the principled roughness volume
    attached = any(isinstance(t, torch.Tensor) and t.requires_grad for t in (data, p, albedo, rough))
    if not (attached and torch.is_grad_enabled()):
        # nothing to differentiate: a plain primal render (no gradient sweep is enqueued)
        if not grid.in_sync_with(data):
            grid.update(data)
        if p is not None:
            grid.set_translation(p)
        return render_forward(grid, sensors, int(spp), seeds=[int(seed) + i for i in range(len(sensors))], integrator=integrator,
                              reparam=reparam, shading=shading)
    return _RenderOp.apply(data, grid, sensors, int(spp), int(seed), int(spp_grad or spp), int(seed_grad),
                           integrator, reparam, p, albedo, shading, rough)
