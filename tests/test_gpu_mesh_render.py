"""GPU parity of the primal mesh render (dsdf.mesh_render, csrc/dsdf_bvh.h: k_mesh_render) against the fp64 image oracle composed
in tests/mesh_render_oracle.py: the project's forward gate, relative L2 <= 1e-4, through precision.image_rel_l2_but_flips with at
most two windows set aside (a ray through an edge may go either way in fp32).  16 x 16 film, the 3-camera ring, explicit
fp32-rounded offsets and emitter samples, spp 64 (wave film reduce) and 4 (per-lane splat)."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import mesh_oracle as M
import mesh_render_oracle as R
import precision as P
import sdf_oracle as O

pytestmark = pytest.mark.gpu

W = H = 16
NV = 3
FWD_TOL = 1e-4
INTEGRATORS = {'silhouette': O.SILHOUETTE, 'shading': O.SIMPLE_SHADING, 'direct': O.DIRECT}
ENV = 0.8


@pytest.fixture(scope='module')
def dsdf(built):
    import dsdf as m
    m.load()
    assert torch.cuda.is_available()
    return m


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(triangles, smooth normals, face normals), shifted by +0.5 into the unit cube the sensors look at."""
    import mesh_to_sdf
    if name == 'box':
        v, f = M.box()
    elif name == 'sphere':
        v, f = M.icosphere(0.3, 2, centre=(0.05, -0.02, 0.01))
    else:                                                                     # two disjoint spheres in one soup: they shadow each other
        va, fa = M.icosphere(0.16, 1, centre=(-0.2, 0.0, 0.02))
        vb, fb = M.icosphere(0.13, 1, centre=(0.17, 0.08, -0.05))
        v, f = np.concatenate([va, vb]), np.concatenate([fa, fb + len(va)])
    v = v + np.float32(0.5)
    return v[f], mesh_to_sdf.vertex_normals(v, f, True), mesh_to_sdf.vertex_normals(v, f, False)


@functools.lru_cache(maxsize=None)
def samples(spp):
    n = (W + 4) * (H + 4) * spp
    gens = [torch.Generator().manual_seed(100 * spp + v) for v in range(NV)]
    offsets = torch.stack([torch.rand(n, 2, generator=g) for g in gens])      # float32: what the kernel reads is what the oracle reads
    emitter = torch.stack([torch.rand(n, 2, generator=g) for g in gens])
    return offsets, emitter


def albedo_volume():
    lin = torch.linspace(0, 1, 6)
    z, y, x = torch.meshgrid(lin, lin, lin, indexing='ij')
    return torch.stack([0.3 + 0.6 * x, 0.9 - 0.5 * y, 0.4 + 0.4 * z * x], -1).float().contiguous()


def cameras(dsdf):
    sens = dsdf.get_regular_cameras(NV, resx=W, resy=H)
    cams = [O.Camera.from_params(np.frombuffer(bytes(s.to_struct()), np.float32, 16)) for s in sens]
    return sens, cams


@functools.lru_cache(maxsize=None)
def primaries(name, spp):
    """The camera rays and closest hits of the three views: computed once per (mesh, spp), shared by the integrators and normal modes."""
    import dsdf
    tri = mesh(name)[0]
    _, cams = cameras(dsdf)
    offsets, _ = samples(spp)
    return [R.primary(tri, cams[v], W, H, spp, offsets[v]) for v in range(NV)]


@functools.lru_cache(maxsize=None)
def reference(name, spp, integ, smooth, hide=False):
    import dsdf
    tri, ns, nf = mesh(name)
    nrm = ns if smooth else (None if smooth is None else nf)
    _, cams = cameras(dsdf)
    offsets, emitter = samples(spp)
    prim = primaries(name, spp)
    return np.stack([R.render(tri, nrm, cams[v], W, H, spp, offsets[v], INTEGRATORS[integ], albedo=albedo_volume(), emitter_u=emitter[v],
                              env=ENV, hide_emitters=hide, prim=prim[v]) for v in range(NV)])


def gpu_render(dsdf, name, spp, integ, smooth, hide=False, views=None):
    tri, ns, nf = mesh(name)
    nrm = ns if smooth else (None if smooth is None else nf)
    bvh = dsdf.MeshBvh(torch.from_numpy(tri).cuda(), None if nrm is None else torch.from_numpy(nrm).cuda())
    sens, _ = cameras(dsdf)
    offsets, emitter = samples(spp)
    vs = list(range(NV)) if views is None else views
    sh = dsdf.Shading(albedo_volume().cuda(), ENV, hide_emitters=hide) if integ == 'direct' else None
    return dsdf.mesh_render(bvh, [sens[v] for v in vs], spp, offsets=offsets[vs].cuda(), integrator=INTEGRATORS[integ], shading=sh,
                            emitter_samples=emitter[vs].cuda() if integ == 'direct' else None).cpu().numpy()


def check(img, ref, spp, tag):
    assert img.shape == ref.shape == (NV, H, W, 3)
    for v in range(NV):
        plain, rest, windows = P.image_rel_l2_but_flips(img[v], ref[v], FWD_TOL, spp, max_flips=2)
        print(f'{tag} view {v}: rel-L2 {plain:.3e}, after {len(windows)} window(s) {rest:.3e}')
        assert rest <= FWD_TOL, (tag, v, plain, rest, windows)


# smooth: True = angle-weighted vertex normals, False = face normals stored per corner, None = no stored normals (geometric normal)
CASES = [(m, i, s) for m in ('box', 'sphere') for i in INTEGRATORS for s in (True,)] + \
        [('sphere', 'shading', False), ('sphere', 'shading', None), ('sphere', 'direct', None), ('box', 'direct', None),
         ('two_spheres', 'direct', True), ('two_spheres', 'silhouette', None)]


@pytest.mark.parametrize('spp', [64, 4])
@pytest.mark.parametrize('name,integ,smooth', CASES)
def test_mesh_render_matches_oracle(dsdf, name, integ, smooth, spp):
    ref = reference(name, spp, integ, smooth)
    assert ref.max() > 0.1 and (integ != 'silhouette' or 0.02 < (ref > 0.5).mean() < 0.9)       # the mesh is in view
    check(gpu_render(dsdf, name, spp, integ, smooth), ref, spp, f'{name}/{integ}/smooth={smooth}/spp{spp}')


def test_face_normals_equal_geometric_normals(dsdf):
    """Face normals stored per corner and no stored normals are the same statement up to the rounding of the normalisation."""
    a = gpu_render(dsdf, 'sphere', 64, 'shading', False)
    b = gpu_render(dsdf, 'sphere', 64, 'shading', None)
    assert P.rel_l2(a, b) < 1e-6
    assert P.rel_l2(a, gpu_render(dsdf, 'sphere', 64, 'shading', True)) > 1e-3               # smooth shading is another image


def test_occlusion_and_hidden_emitters(dsdf):
    """hide_emitters blackens the escaping rays, and the two spheres do shadow each other (the oracle without the shadow query differs)."""
    both = reference('two_spheres', 64, 'direct', True)
    hid = reference('two_spheres', 64, 'direct', True, True)
    check(gpu_render(dsdf, 'two_spheres', 64, 'direct', True, hide=True), hid, 64, 'two_spheres/hidden')
    assert np.abs(both[:, 0, 0] - ENV).max() < 1e-12 and np.abs(hid[:, 0, 0]).max() == 0.0
    tri, ns, _ = mesh('two_spheres')
    _, cams = cameras(dsdf)
    offsets, emitter = samples(64)
    unshadowed = R.render(tri, ns, cams[0], W, H, 64, offsets[0], O.DIRECT, albedo=albedo_volume(), emitter_u=emitter[0], env=ENV,
                          prim=primaries('two_spheres', 64)[0], occlusion=False)
    assert P.rel_l2(unshadowed, both[0]) > 10 * FWD_TOL                                       # the shadows are part of what is compared


def test_batch_equals_single_views_and_builtin_sampler(dsdf):
    img = gpu_render(dsdf, 'sphere', 64, 'direct', True)
    for v in range(NV):
        one = gpu_render(dsdf, 'sphere', 64, 'direct', True, views=[v])
        assert P.rel_l2(one[0], img[v]) < 1e-6
    # the built-in sampler draws what dsdf_sampler_2d reports (film) and the emitter samples of the SDF render (later dimensions)
    tri, ns, _ = mesh('sphere')
    bvh = dsdf.MeshBvh(torch.from_numpy(tri).cuda(), torch.from_numpy(ns).cuda())
    sens, _ = cameras(dsdf)
    n = (W + 4) * (H + 4) * 4
    offs = torch.stack([torch.tensor(O.independent_sampler_2d(5 + i, n)) for i in range(NV)]).float().cuda()
    emit = torch.stack([torch.tensor(O.independent_sampler_emitter_2d(5 + i, n)) for i in range(NV)]).float().cuda()
    sh = dsdf.Shading(albedo_volume().cuda(), ENV)
    a = dsdf.mesh_render(bvh, sens, 4, seeds=[5, 6, 7], integrator='sdf_direct_reparam', shading=sh)
    b = dsdf.mesh_render(bvh, sens, 4, offsets=offs, integrator='sdf_direct_reparam', shading=sh, emitter_samples=emit)
    assert P.rel_l2(a.cpu().numpy(), b.cpu().numpy()) < 1e-6


def test_argument_validation(dsdf):
    lib = dsdf.load()
    p = dsdf.default_params()
    cam = (dsdf.DsdfCamera * 1)()
    one = C.c_void_p(16)                                                      # never dereferenced: validation fails first
    seeds = (C.c_uint32 * 1)(1)
    big = 1 << 30
    assert lib.dsdf_mesh_render_workspace_size(16, 16, 1) == 20 * 20 * 16 and lib.dsdf_mesh_render_workspace_size(0, 16, 1) == 0
    assert lib.dsdf_mesh_render_workspace_size(16, 16, 100) == 16 * 20 * 20 * 16
    sh = dsdf.DsdfShading()
    sh.albedo, sh.ax, sh.ay, sh.az = 16, 2, 2, 2

    def call(bvh=one, integ=0, ws=big, shading=None, sd=seeds):
        return lib.dsdf_mesh_render_forward(bvh, C.byref(p), cam, 1, 16, 16, 4, None, sd, integ, shading, one, one, ws, None)
    for kwargs, want, text in [(dict(bvh=None), -1, b'null pointer'), (dict(integ=7), -1, b'unknown integrator'),
                               (dict(ws=16), -2, b'workspace too small'), (dict(integ=2), -1, b'dsdf_shading'),
                               (dict(sd=None), -1, b'need offsets or seeds')]:
        assert call(**kwargs) == want and text in lib.dsdf_last_error() and b'dsdf_mesh_render_forward' in lib.dsdf_last_error(), kwargs
    sh.use_mis = 1
    assert call(integ=2, shading=C.byref(sh)) == -1 and b'dsdf_mesh_render_forward' in lib.dsdf_last_error() and b'use_mis' in lib.dsdf_last_error()
    sh.use_mis, sh.bsdf = 0, 1
    assert call(integ=2, shading=C.byref(sh)) == -1 and b'dsdf_mesh_render_forward' in lib.dsdf_last_error() and b'bsdf' in lib.dsdf_last_error()
    with pytest.raises(dsdf.DsdfError, match='no CPU path'):
        dsdf.MeshBvh(torch.zeros(4, 3, 3))


def test_optimize_cli_with_mesh_references(dsdf, tmp_path, monkeypatch):
    """`optimize.py ball --optconfig no-tex-2 --meshrefs`: the reference images are rendered from scenes/ball/ball.obj itself, under
    the usual names, and the optimisation runs against them."""
    import optimize
    import scenes
    v, f = M.icosphere(0.3, 2)
    d = tmp_path / 'scenes' / 'ball'
    d.mkdir(parents=True)
    M.write_obj(str(d / 'ball.obj'), v, f)
    monkeypatch.setattr(scenes, 'SCENE_DIR', str(tmp_path / 'scenes'))
    monkeypatch.setattr(optimize, 'RENDER_DIR', str(tmp_path / 'renders'))
    tri, nrm = scenes.load_target_mesh('ball')
    assert tri.shape == (320, 3, 3) and nrm.shape == (320, 3, 3) and tri.is_cuda
    assert abs(float(tri.mean()) - 0.5) < 1e-3 and scenes.load_target_mesh('nothing_here') is None
    centre = tri.mean(1) - 0.5
    assert float((torch.nn.functional.normalize(centre, dim=1) * nrm[:, 0]).sum(1).min()) > 0.9      # outward vertex normals
    optimize.main(['ball', '--optconfig', 'no-tex-2', '--configs', 'warp', '--outputdir', str(tmp_path / 'out'), '--refspp', '64', '--n_iter=2',
                   '--spp=64', '--sdf_res=32', '--integrator=sdf_silhouette_reparam', '--resx=32', '--resy=32', '--meshrefs'])
    out = tmp_path / 'out' / 'ball' / 'no-tex-2' / 'warp'
    lv = json.load(open(out / 'metadata.json'))['loss_values']
    assert len(lv) == 2 and all(np.isfinite(lv)), lv
    refs = sorted((tmp_path / 'renders').rglob('ref-*.npy'))
    assert refs and (out / 'ref-00.npy').exists()
    ref0 = np.load(out / 'ref-00.npy')
    cov = (ref0 > 0.5).mean()
    assert ref0.shape == (32, 32, 3) and 0.02 < cov < 0.6                                       # a ball of radius 0.3 in view
